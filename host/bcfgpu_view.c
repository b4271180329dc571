/*  bcfgpu_view.c -- format conversion on the pipe boundary: VCF / bgzipped VCF / BCF2 in, any of them out (what
 *  `bcftools view [-O v|z|u|b]` does for a file that needs no filtering; used the way test.pl:1194-1195 uses it, to turn
 *  the BCF output of the drivers back into text).
 *
 *      bcfgpu_view [-O v|z|u|b] [-o out] [-H] [--int-columns] [--lazy] [--key-blocks] <in|->            -H: records only, no header
 *  --int-columns: a record whose per-sample columns are all integers (no GT, no '.' inside a vector but as a whole value) is written
 *  through vio_write_record_int -- the columns as integer arrays, the way host/bcfgpu_sam hands them over -- instead of as its text
 *  line; the output must not differ (tests/test_vcfio.py).
 *  --lazy: BCF input is read through vio_read_record + vio_indiv_text -- the head and the sample columns decoded apart, the way
 *  host/bcfgpu_call --device-input reads -- instead of vio_read_line; the output must not differ (tests/test_vcfio_lazy.py).
 *  --key-blocks: with BCF output, a record with samples is written as its head and the per-sample part put together from the FORMAT keys'
 *  blocks, each made on its own by vio_encode_keys (every key with its values cut out of the sample columns), through
 *  vio_write_record_indiv -- the way host/bcfgpu_call --device-records writes -- instead of as its text line; the output must not
 *  differ (tests/test_call_indiv_encoder.py).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <ctype.h>
#include "vcfio.h"


/* 0: the record went out through vio_write_record_int; 1: it does not qualify (the caller writes the text line) */
static int int_pad = 0;         /* --int-columns-pad N: the columns handed over N values wider than any sample needs (a caller with fixed-width planes) */
static int write_int_columns(vio_file *fo, const vio_hdr *h, char *line, long *n_done)
{
    const int S = vio_hdr_nsamples(h);
    char *f8 = line; int tabs = 0;
    for (char *p = line; *p; ++p) if (*p == '\t' && ++tabs == 8) { f8 = p + 1; break; }
    if (tabs < 8 || !S) return 1;
    char *smp = strchr(f8, '\t');
    if (!smp) return 1;
    int nk = 1; for (char *p = f8; p < smp; ++p) if (*p == ':') ++nk;
    if (nk > 32 || (smp - f8 >= 2 && !strncmp(f8, "GT", 2) && (f8[2] == ':' || f8 + 2 == smp))) return 1;
    /* widths: the largest number of values any sample has for the key */
    int width[32]; for (int k = 0; k < nk; ++k) width[k] = 1;
    const char *q = smp + 1;
    for (int s = 0; s < S; ++s) {
        int k = 0, w = 1;
        for (;; ++q) {
            if (*q == ',') ++w;
            else if (*q == ':' || *q == '\t' || !*q) { if (k < nk && w > width[k]) width[k] = w; ++k; w = 1; if (*q != ':') break; }
            else if (!isdigit((unsigned char)*q) && *q != '-' && *q != '.') return 1;
        }
        if (k != nk) return 1;                                 /* trailing fields dropped: leave it to the text path */
        if (*q) ++q;
    }
    int32_t *col[32];
    for (int k = 0; k < nk; ++k) { width[k] += int_pad; col[k] = malloc((size_t)S * (size_t)width[k] * 4); }
    q = smp + 1;
    int ok = 1;
    for (int s = 0; s < S && ok; ++s)
        for (int k = 0; k < nk; ++k) {
            int j = 0;
            for (;;) {
                char *e; long v;
                if (*q == '.') { v = VIO_INT_MISSING; e = (char *)q + 1; } else v = strtol(q, &e, 10);
                if (e == q) { ok = 0; break; }
                col[k][(size_t)s * width[k] + j++] = (int32_t)v;
                q = e;
                if (*q == ',') { ++q; continue; }
                break;
            }
            for (; j < width[k]; ++j) col[k][(size_t)s * width[k] + j] = VIO_INT_VEND;
            if (*q == ':' || *q == '\t') ++q;
        }
    int rc = 1;
    if (ok) {
        *smp = 0;                                                /* the head: CHROM .. FORMAT */
        rc = vio_write_record_int(fo, h, line, nk, width, (const int32_t *const *)col) ? 1 : 0;
        if (rc) { *smp = '\t'; }
        else ++*n_done;
    }
    for (int k = 0; k < nk; ++k) free(col[k]);
    return rc;
}

/* --key-blocks: 0: the record went out as head + key blocks; 1: it has no sample columns (the caller writes the text line); -1: error */
static int write_key_blocks(vio_file *fo, const vio_hdr *h, char *line)
{
    const int S = vio_hdr_nsamples(h);
    char *f8 = NULL; int tabs = 0;
    for (char *p = line; *p; ++p) if (*p == '\t' && ++tabs == 8) { f8 = p + 1; break; }
    char *smp = f8 ? strchr(f8, '\t') : NULL;
    if (!smp || !S) return 1;
    *smp = 0;                                                    /* the head: CHROM .. FORMAT */
    int nk; char *fmt = strdup(f8), *keys[64];
    nk = 0; for (char *t = strtok(fmt, ":"); t && nk < 64; t = strtok(NULL, ":")) keys[nk++] = t;
    /* every key alone: its values of all samples as one-key sample columns, its block appended to the record's */
    char *all = NULL, *one = NULL, *cols = malloc(strlen(smp + 1) + 2); size_t l_all = 0, m_all = 0, cap1 = 0, end[64];
    int rc = 0;
    for (int k = 0; k < nk && !rc; ++k) {
        char *o = cols; const char *q = smp + 1;
        for (int s = 0; s < S; ++s) {
            const char *e = strchr(q, '\t'); if (!e) e = q + strlen(q);
            const char *v = q; int i = 0;
            while (i < k && v) { const char *c = memchr(v, ':', (size_t)(e - v)); v = c ? c + 1 : NULL; ++i; }
            if (s) *o++ = '\t';
            if (!v) *o++ = '.';
            else { const char *c = memchr(v, ':', (size_t)(e - v)); if (!c) c = e; memcpy(o, v, (size_t)(c - v)); o += c - v; }
            q = *e ? e + 1 : e;
        }
        *o = 0;
        if (vio_encode_keys(h, keys[k], cols, S, &one, &cap1, end) != 1) { rc = -1; break; }
        if (l_all + end[0] > m_all) { m_all = (l_all + end[0]) * 2 + 64; all = realloc(all, m_all); }
        memcpy(all + l_all, one, end[0]); l_all += end[0];
    }
    if (!rc && vio_write_record_indiv(fo, h, line, all ? all : "", l_all)) rc = -1;
    free(all); free(one); free(cols); free(fmt);
    return rc;
}

int main(int argc, char **argv)
{
    char mode = 'v'; const char *out = "-", *in = NULL; int no_hdr = 0, int_cols = 0, lazy = 0, key_blocks = 0;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "-O") && i + 1 < argc) mode = argv[++i][0];
        else if (!strncmp(argv[i], "-O", 2) && argv[i][2]) mode = argv[i][2];
        else if (!strcmp(argv[i], "-o") && i + 1 < argc) out = argv[++i];
        else if (!strcmp(argv[i], "-H")) no_hdr = 1;
        else if (!strcmp(argv[i], "--int-columns")) int_cols = 1;
        else if (!strcmp(argv[i], "--lazy")) lazy = 1;
        else if (!strcmp(argv[i], "--key-blocks")) key_blocks = 1;
        else if (!strcmp(argv[i], "--int-columns-pad") && i + 1 < argc) { int_cols = 1; int_pad = atoi(argv[++i]); }
        else in = argv[i];
    }
    if (!in) { fprintf(stderr, "usage: bcfgpu_view [-O v|z|u|b] [-o out] [-H] [--int-columns] [--lazy] [--key-blocks] <in|->\n"); return 2; }
    vio_file *fi = vio_open_read(in);
    if (!fi) { fprintf(stderr, "%s\n", vio_error()); return 1; }
    vio_hdr *h = vio_read_hdr(fi);
    if (!h) { fprintf(stderr, "%s\n", vio_error()); return 1; }
    vio_file *fo = vio_open_write(out, mode);
    if (!fo) { fprintf(stderr, "%s\n", vio_error()); return 1; }
    if (!no_hdr && vio_write_hdr(fo, h)) { fprintf(stderr, "%s\n", vio_error()); return 1; }
    char *line = NULL; size_t cap = 0; int rc;
    long n_int = 0;
    char *text = NULL; size_t tcap = 0;
    for (;;) {
        if (lazy) {
            const void *indiv; size_t l_indiv; int n_fmt, n_sample;
            if ((rc = vio_read_record(fi, h, &line, &cap, &indiv, &l_indiv, &n_fmt, &n_sample)) <= 0) break;
            if (vio_indiv_text(h, indiv, l_indiv, n_fmt, n_sample, &text, &tcap)) { rc = -1; break; }
            const size_t hl = strlen(line), tl = strlen(text);
            if (hl + tl + 1 > cap) { cap = hl + tl + 1; line = realloc(line, cap); }
            memcpy(line + hl, text, tl + 1);
        } else if ((rc = vio_read_line(fi, h, &line, &cap)) <= 0) break;
        if (int_cols && write_int_columns(fo, h, line, &n_int) == 0) continue;
        if (key_blocks && (mode == 'u' || mode == 'b')) {
            const int kb = write_key_blocks(fo, h, line);
            if (kb < 0) { fprintf(stderr, "%s\n", vio_error()); return 1; }
            if (kb == 0) continue;
        }
        if (vio_write_line(fo, h, line)) { fprintf(stderr, "%s\n", vio_error()); return 1; }
    }
    if (int_cols) fprintf(stderr, "%ld records written from integer columns\n", n_int);
    if (rc < 0) { fprintf(stderr, "%s\n", vio_error()); return 1; }
    free(line); free(text);
    if (vio_close(fo)) { fprintf(stderr, "%s\n", vio_error()); return 1; }
    vio_close(fi); vio_hdr_free(h);
    return 0;
}
