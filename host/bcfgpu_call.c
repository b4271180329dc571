/*  bcfgpu_call.c -- `bcftools call -m [-v]` over a VCF from `bcftools mpileup`, in plain C over the C-ABI of
 *  include/bcfgpu.h: the record loop of main_vcfcall (vcfcall.c:1089-1148) with mcall() on the device.
 *
 *      bcfgpu_call [-v] [-S samples.txt | -s NAME,...] [--ploidy-file file | --ploidy GRCh37|GRCh38|X|Y|1] [-G -|groups.txt [--group-samples-tag TAG]]
 *                  [-F AN_TAG,AC_TAG] [-a GQ,GP] [--device-input] [--device-parse] [--device-alleles] [--device-records] [--device-keys] [--device-text] [--timing] [-O v|z|u|b] <in.vcf>
 *          -S: the samples to keep, in that order: NAME [PLOIDY|SEX] per line, or a PED file (vcfcall.c:202-344)
 *          --ploidy-file: CHROM FROM TO SEX PLOIDY lines, '*' = default for the sex (ploidy.c).  The definition also sets the prior's
 *              allele count: ploidy_max() of it times the samples (vcfcall.c:652-656) -- one a sample with --ploidy 1, else two
 *          -G: sample groups with their own allele frequencies, '-' = every sample alone, or NAME GROUP lines
 *              (mcall.c:258-345); the frequencies come from FORMAT/QS or FORMAT/AD (--group-samples-tag)
 *          -F: INFO tags holding AN and AC of a prior population (mcall.c:1499-1520)
 *          -a: FORMAT/GQ and FORMAT/GP on called variant records (mcall.c:1618-1623)
 *          --device-input: BCF input is not turned into text and back: the records' per-sample blocks go to the device as the file
 *              holds them and bcfgpu_call_decode_bcf makes the PL (and, with -G, AD / QS) planes there; the sample columns become
 *              text only for the records that are written.  Takes effect on BCF input without -C alleles (but see --device-alleles) and
 *              without -g (both read the samples' values on the host); in any other run the option does nothing.  The same output either way.
 *          --device-parse: the same for VCF text input (plain, bgzipped or on a pipe): a line is split at its first nine tabs only, the
 *              rest of it -- the sample columns, from their tab on -- goes to the device as text and bcfgpu_call_decode_vcf parses the PL
 *              (and, with -G, AD / QS) planes there; a record's columns are split on the host only when the record is written.  Takes
 *              effect on text input without -C alleles (but see --device-alleles) and without -g; in any other run the option does nothing, and it may stand
 *              beside --device-input (each acts on its own kind of input).  Stricter than the host's atoi: a PL / AD / QS value that is
 *              not '.' or [+-]?[0-9]+ inside int32 is "malformed VCF".  The same output either way.
 *          --device-alleles: with -C alleles -T targets, where --device-input (BCF in) or --device-parse (text in) is given and would act
 *              but for -C alleles: that option takes effect.  The host keeps the head of the rewrite -- the pairing with a target, amap,
 *              REF / ALT, INFO/QS, the -i lines -- and runs it on the record's first nine columns; the samples' bytes or text go to the
 *              device untouched, the decoders make planes of the input records' shape there, and bcfgpu_call_constrain gathers them into
 *              the planes mcall() reads (PL through pl_map with the unseen allele standing in; with -G the tag's planes through amap).
 *              A written record's sample text, where the host still forms it, comes from the input's own bytes or text: PL is printed from
 *              the planes, the other Number=R keys of a changed record go through amap first, then als_map.  --device-records,
 *              --device-keys and --device-text act as without -C alleles, but a Number=R key other than PL of a changed record is the
 *              host's (--device-keys: no job; --device-text: the record's columns are formed on the host): those kernels apply als_map to
 *              the input's own vector.  In any other run the option does nothing.  The same output either way.
 *          --device-records: with -O u|b the records' GT, PL and GQ do not come down as planes to be printed and parsed back: after the
 *              calls bcfgpu_call_encode_bcf turns them into BCF2 key blocks in HBM, for the records that are written only, and the host
 *              downloads the site records, the bytes and one offset per record and key.  A record is then its head and
 *              vio_write_record_indiv of the blocks in the text route's order: GT (device), the input's keys with the device's PL
 *              block in PL's place (nothing when PL is dropped) and the other keys' blocks made on the host from their text
 *              (vio_encode_keys; Number=R tags trimmed as ever), GP (host: its bytes are those of the "%g" text), GQ (device).
 *              Does nothing with -O v|z and with -g (whose block lines read the genotypes on the host).  The same output either way.
 *          --device-keys: with --device-input and --device-records both in effect, the integer keys the caller passes through (AD, ADF,
 *              ADR, DP, SP, ...: declared Type=Integer, not PL, not GT, stored as int8 / int16 / int32 or without values, at most 255
 *              values a sample) are not printed, split, re-ordered and parsed back either: the input records' bytes stay in HBM after
 *              the decode and bcfgpu_call_remap_bcf makes those keys' blocks of the written records there -- the -S sample choice,
 *              the Number=R values following als_map, width and type chosen anew -- one size call and one write call over all of
 *              them.  The host splices them in their keys' places; Float and String keys and GP stay on the host
 *              (vio_encode_keys), and a record without any of those forms no sample text at all.
 *              With --device-parse and --device-records both in effect (text in, BCF out) the same for VCF text input: the columns'
 *              text stays in HBM after the decode and bcfgpu_call_parse_keys_vcf makes the blocks there from every written record's
 *              own columns -- a job for each key of the FORMAT column that the header declares Type=Integer, that is not PL, not
 *              named GT and stands among the first 64 keys; token by token, the exact integer grammar, the -S sample choice, the
 *              Number=R values following als_map, width and type chosen anew.  A key one of whose values the grammar refuses (an
 *              empty value, `12x`, a blank, a number past int32: strtol makes something of each) or that is wider than 255 values
 *              comes back flagged and is the host's again, with Float and String keys and GP: the host's text of a record holds only
 *              those keys' tokens, and a record with integer keys alone and no GP has no column copied or split.
 *              In any other run the option does nothing.  The same output either way.
 *          --device-text: with -O v|z and --device-input in effect, the sample columns of the written records are not formed on the
 *              host either: the input records' bytes stay in HBM after the decode and bcfgpu_call_encode_vcf formats every such
 *              record's columns there -- GT, the input's keys in their order with the trimmed PL in PL's place (nothing when PL is
 *              dropped), the -S sample choice, the Number=R values following als_map, GQ -- one size call and one write call over
 *              all of them.  The host prints the head up to the FORMAT column and hands both to vio_write_record_text.  A record
 *              stays on the host (the route without options) when an input key other than PL is not stored as integers of at most
 *              255 values, a key is named GT, the record carries GP, or it has more than 16 fields or passes the bound of
 *              include/bcfgpu.h; when no written record does, the GT, PL and GQ planes are not downloaded.
 *              With -O v|z and --device-parse in effect (text in, text out) the same for VCF text input: the columns' text stays in
 *              HBM after the decode and bcfgpu_call_rewrite_vcf rewrites every written record's columns there, token by token -- GT
 *              in front, the trimmed PL in PL's place (nothing when PL is dropped), the -S sample choice, the Number=R tokens
 *              following als_map, every other token as the bytes it is, GQ behind.  A Float or String key keeps no record from the
 *              device here; a record stays on the host when it carries GP, a key is named GT, or it has more than 64 FORMAT keys.
 *              In any other run the option does nothing.  The same output either way.
 *          --timing: lines on stderr: the seconds (reading records, building the planes on the host, uploads and device stages,
 *              writing records), how many records' planes were decoded on the device, and how many records' FORMAT blocks were
 *              encoded there; with --device-parse given, also how many records' planes were parsed on the device; with --device-keys given, also how many pass-through key blocks were made on the device and on the host;
 *              with --device-text given, also how many records' sample columns were formatted on the device and on the host;
 *              with --device-alleles given, also how many records' planes were constrained on the device and how many were taken as they were
 *
 *  Host: VCF text in, what mcall() reads from a record (alleles, FORMAT/PL, INFO/QS, INFO/I16) packed into the planes of
 *  bcfgpu_call_in, one bcfgpu_mcall over all records, then what mcall.c:1627-1681 does to the record: alleles trimmed with
 *  als_map, GT in front of the FORMAT fields, PL trimmed (or dropped), QUAL, INFO/AC, AN, DP4, MQ appended, I16 and QS
 *  removed.  Prints the data lines of the output VCF; tests/test_c_host.py compares them, byte for byte, with the
 *  reference's goldens of `call -m` (test.pl:276-308: mpileup.{1,3,4,5}, mpileup.X{,.2}, mpileup.hwe.*, call-G.*,
 *  call.af-fixation.*).
 *  Number=R tags of INFO and FORMAT follow the alleles (mcall_trim_and_update_numberR, mcall.c:1196-1265).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <stdint.h>
#include <stdarg.h>
#include "bcfgpu.h"
#include "vcfio.h"
#include "drv.h"

/* with --device-input: line = the first nine columns, the per-sample block = ilen bytes at ioff of the byte buffer, its key headers in keys;
 * with --device-parse: line = the first nine columns, the sample columns' text (from the ninth tab on) = ilen bytes at ioff */
typedef struct { char *line; char **fld; int nfld; char **als; int nals, unseen, pl_idx, ad_idx; uint8_t *ploidy;
                 size_t ioff, ilen; int n_fmt, nkeys; vio_indiv_key *keys;
                 int *kjob, nkjob;              /* --device-keys, a written record: key i's job of bcfgpu_call_remap_bcf (text input: of
                                                 * bcfgpu_call_parse_keys_vcf), or -1 (the host's); nkjob entries, one a FORMAT key */
                 int nori, unseen_in, changed, amap[BCFGPU_MAX_ALLELES]; } rec_t;   /* --device-alleles: the input record's allele count and unseen
                                                 * allele, whether -C alleles changes it, new allele -> original allele (bcfgpu_cals_site) */

typedef struct { char chrom[256]; int from, to, ploidy; char sex[64]; } preg_t;

static char **split(char *s, char sep, int *n)
{
    int cap = 8; char **v = malloc((size_t)cap * sizeof *v); *n = 0;
    for (;;) {
        if (*n == cap) { cap *= 2; v = realloc(v, (size_t)cap * sizeof *v); }
        v[(*n)++] = s;
        s = strchr(s, sep);
        if (!s) break;
        *s++ = 0;
    }
    return v;
}

/* the Number=R tags the header declares (they follow the alleles when some are dropped) */
static char infoR[64][64], fmtR[64][64];
static int n_infoR = 0, n_fmtR = 0, has_fmt_qs = 0, has_fmt_ad = 0;

static void header_line(const char *ln)
{
    const int is_info = !strncmp(ln, "##INFO=<ID=", 11), is_fmt = !strncmp(ln, "##FORMAT=<ID=", 13);
    if (!is_info && !is_fmt) return;
    const char *id = ln + (is_info ? 11 : 13), *e = strchr(id, ',');
    if (is_fmt && e && e - id == 2) { has_fmt_qs |= !strncmp(id, "QS", 2); has_fmt_ad |= !strncmp(id, "AD", 2); }
    if (!e || !strstr(e, "Number=R") || e - id > 63) return;
    char (*tab)[64] = is_info ? infoR : fmtR; int *cnt = is_info ? &n_infoR : &n_fmtR;
    if (*cnt == 64) return;
    memcpy(tab[*cnt], id, (size_t)(e - id)); tab[*cnt][e - id] = 0; ++*cnt;
}

static int is_numberR(char (*tab)[64], int cnt, const char *key, size_t klen)
{
    for (int i = 0; i < cnt; ++i) if (strlen(tab[i]) == klen && !strncmp(tab[i], key, klen)) return 1;
    return 0;
}

/* a comma-separated Number=R value list with the kept alleles' values in their new places */
static void print_numberR(const char *vals, const int32_t *als_map, int nals, int nn)
{
    char *c = strdup(vals); int nv; char **v = split(c, ',', &nv);
    if (nv != nals) fputs(vals, LN);                        /* '.', or not one value per allele: left alone */
    else if (nn == 1) fputs(v[0], LN);
    else {
        const char *o[5] = { ".", ".", ".", ".", "." };
        for (int i = 0; i < nals; ++i) if (als_map[i] >= 0) o[als_map[i]] = v[i];
        for (int i = 0; i < nn; ++i) fprintf(LN, "%s%s", i ? "," : "", o[i]);
    }
    free(v); free(c);
}

/* ---- call -C alleles -T targets [-i]: the record is re-expressed in the alleles of the target file before mcall() sees it
 * (mcall_constrain_alleles, mcall.c:1271-1421), the target line is chosen as next_line() does (vcfcall.c:501-605) with the
 * allele comparison of vcmp.c:55-119, and -i writes a line for every target that met no record (tgt_flush, vcfcall.c:408-455).
 * Host logic on the record text; the call itself is the device's, with -A. ---- */
typedef struct { char *chrom; int pos; char **als; int nals, used, order; } tgt_t;
static tgt_t *tgt = NULL; static int n_tgt = 0; static int *tgt_sorted = NULL;
static int cals = 0, insert_missed = 0;

static void tgt_parse(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) DIE("cannot open %s\n", path);
    char ln[1 << 16], c[256], a[1 << 15]; int pos;
    while (fgets(ln, sizeof ln, f)) {
        if (sscanf(ln, "%255s %d %32767s", c, &pos, a) != 3) continue;
        tgt = realloc(tgt, (size_t)(n_tgt + 1) * sizeof *tgt);
        tgt_t *t = &tgt[n_tgt];
        t->chrom = strdup(c); t->pos = pos; t->used = 0; t->order = n_tgt;
        char *al = strdup(a); t->als = split(al, ',', &t->nals);
        ++n_tgt;
    }
    fclose(f);
    /* the regions of a sequence sorted by start (regidx), sequences in the order they first appear */
    tgt_sorted = malloc((size_t)(n_tgt ? n_tgt : 1) * sizeof *tgt_sorted);
    int m = 0;
    for (int i = 0; i < n_tgt; ++i) {
        int seen = 0;
        for (int j = 0; j < i; ++j) if (!strcmp(tgt[j].chrom, tgt[i].chrom)) { seen = 1; break; }
        if (seen) continue;
        const int m0 = m;
        for (int j = i; j < n_tgt; ++j) if (!strcmp(tgt[j].chrom, tgt[i].chrom)) tgt_sorted[m++] = j;
        for (int x = m0 + 1; x < m; ++x)                        /* stable insertion sort by position */
            for (int y = x; y > m0 && tgt[tgt_sorted[y]].pos < tgt[tgt_sorted[y - 1]].pos; --y) { const int t = tgt_sorted[y]; tgt_sorted[y] = tgt_sorted[y - 1]; tgt_sorted[y - 1] = t; }
    }
}
static size_t common_prefix_ci(const char *a, const char *b)
{
    size_t i = 0;
    while (a[i] && b[i] && (a[i] & ~32) == (b[i] & ~32) && ((a[i] | 32) >= 'a' && (a[i] | 32) <= 'z' ? 1 : a[i] == b[i])) ++i;
    return i;
}
static int ci_equal(const char *a, const char *b) { while (*a && *b) { char x = *a, y = *b; if (x >= 'a' && x <= 'z') x -= 32; if (y >= 'a' && y <= 'z') y -= 32; if (x != y) return 0; ++a; ++b; } return !*a && !*b; }
/* vcmp_set_ref / vcmp_find_allele: the difference of the two REF strings, then allele matching modulo that suffix */
typedef struct { int ndref; const char *dref; } vcmp_t;
static int vcmp_set_ref(vcmp_t *v, const char *r1, const char *r2)
{
    v->ndref = 0; v->dref = "";
    const size_t i = common_prefix_ci(r1, r2), l1 = strlen(r1), l2 = strlen(r2);
    if (i == l1 && i == l2) return 0;
    if (i < l1 && i < l2) return -1;
    if (i < l1) { v->dref = r1 + i; v->ndref = (int)(l1 - i); } else { v->dref = r2 + i; v->ndref = -(int)(l2 - i); }
    return 0;
}
static int vcmp_find_allele(const vcmp_t *v, char **als1, int n1, const char *al2)
{
    for (int i = 0; i < n1; ++i) {
        const char *a = als1[i];
        const size_t k = common_prefix_ci(a, al2), la = strlen(a), lb = strlen(al2);
        if (k < la && k < lb) continue;
        if (!v->ndref) { if (k == la && k == lb) return i; continue; }
        if (k < la) { if (v->ndref < 0 || !ci_equal(a + k, v->dref)) continue; return i; }
        if (v->ndref > 0 || !ci_equal(al2 + k, v->dref)) continue;
        return i;
    }
    return -1;
}
static int als_is_indel(char **als, int n)                     /* vcfcall.c:456-470 */
{
    if (n > 1 && als[1][0] == '<') return 0;
    for (int i = 0; i < n; ++i) if (als[i][0] != '<' && strlen(als[i]) > 1) return 1;
    return 0;
}
static int gt_index(int a, int b) { return a > b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; }
static void gt_alleles(int igt, int *a, int *b) { int k = 0; while ((k + 1) * (k + 2) / 2 <= igt) ++k; *b = k; *a = igt - k * (k + 1) / 2; }

/* the -i lines of the targets in [beg0, end0] of `chrom` that met no record, appended to the event list */
typedef struct { int is_missed; int tgt; } event_t;             /* is_missed: print target `tgt`; else: record (index in recs) */
static event_t *events = NULL; static int n_events = 0;
static void push_event(int is_missed, int idx) { events = realloc(events, (size_t)(n_events + 1) * sizeof *events); events[n_events].is_missed = is_missed; events[n_events++].tgt = idx; }
static void flush_region(const char *chrom, long beg0, long end0)
{
    for (int x = 0; x < n_tgt; ++x) {
        tgt_t *t = &tgt[tgt_sorted[x]];
        if (strcmp(t->chrom, chrom) || t->pos - 1 < beg0 || t->pos - 1 > end0 || t->used) continue;
        t->used = 1;
        push_event(1, tgt_sorted[x]);
    }
}

typedef struct { char *p; size_t o, cap; } obuf_t;              /* the line constrain_line writes */
static void outf(obuf_t *b, const char *fmt, ...) { va_list ap; va_start(ap, fmt); b->o += (size_t)vsnprintf(b->p + b->o, b->cap - b->o, fmt, ap); va_end(ap); }
/* -C alleles, the head of the rewrite: what needs the record's first nine columns and the target alone (mcall.c:1271-1331, :1372-1379) --
 * amap (new allele -> original allele), the new alleles, whether anything changes */
typedef struct { int nori, nals, unseen, changed, amap[8]; const char *als[8]; char *unseen_al; } chead_t;
/* f: the record's columns, alts: its ALT alleles; 0, or -1 when mcall() would return -2 (the site is skipped, mcall.c:1294-1303) */
static int constrain_head(char **f, char **alts, int nalt, const tgt_t *t, int unseen, chead_t *h)
{
    if (t->nals > 5) DIE("Maximum accepted number of alleles is 5\n");
    vcmp_t vc;
    if (vcmp_set_ref(&vc, f[3], t->als[0]) < 0) DIE("The reference alleles are not compatible at %s:%s\n", f[0], f[1]);
    int nals = 1, has_new = 0;
    h->nori = 1 + nalt; h->unseen = unseen; h->unseen_al = NULL;
    h->amap[0] = 0; h->als[0] = t->als[0];
    for (int i = 1; i < t->nals; ++i) {
        const int j = vcmp_find_allele(&vc, alts, nalt, t->als[i]);
        if (j + 1 == unseen) return -1;                                                   /* mcall.c:1294-1303 */
        if (j >= 0) h->amap[nals] = j + 1; else { h->amap[nals] = unseen >= 0 ? unseen : h->nori - 1; has_new = 1; }
        h->als[nals++] = t->als[i];
    }
    if (unseen) { h->amap[nals] = unseen; h->unseen_al = strdup(unseen == 0 ? f[3] : alts[unseen - 1]); h->als[nals++] = h->unseen_al; }
    h->nals = nals; h->changed = has_new || nals != h->nori;
    return 0;
}
/* the first nine columns of a changed record: REF and ALT are the target's, INFO/QS follows the alleles (absent alleles: 0) */
static void constrained_columns(obuf_t *ob, char **f, const chead_t *h)
{
    const int nals = h->nals;
    outf(ob, "%s\t%s\t%s\t%s\t", f[0], f[1], f[2], h->als[0]);
    if (nals == 1) outf(ob, "."); else for (int i = 1; i < nals; ++i) outf(ob, "%s%s", i > 1 ? "," : "", h->als[i]);
    outf(ob, "\t%s\t%s\t", f[5], f[6]);
    int ni; char *info = strdup(f[7]), **iv = split(info, ';', &ni);
    for (int i = 0; i < ni; ++i) {
        if (i) outf(ob, ";");
        if (!strncmp(iv[i], "QS=", 3)) {
            int nq; char *qc = strdup(iv[i] + 3), **qv = split(qc, ',', &nq);
            outf(ob, "QS=");
            for (int k = 0; k < nals; ++k) outf(ob, "%s%.9g", k ? "," : "", h->amap[k] < nq ? (double)(float)atof(qv[h->amap[k]]) : 0.);
            free(qv); free(qc);
        } else outf(ob, "%s", iv[i]);
    }
    free(iv); free(info);
    outf(ob, "\t%s", f[8]);
}
/* a Number=R token in the new alleles: new[k] = old[amap[k]], '.' where the token has no such value; a '.' token is left alone */
static void constrained_numberR(obuf_t *ob, const char *tok, const int *amap, int nals)
{
    if (!strcmp(tok, ".")) { outf(ob, "."); return; }
    int nv; char *vc2 = strdup(tok), **vv = split(vc2, ',', &nv);
    for (int a = 0; a < nals; ++a) outf(ob, "%s%s", a ? "," : "", amap[a] < nv ? vv[amap[a]] : ".");
    free(vv); free(vc2);
}
/* the sample columns of a changed record (mcall.c:1332-1371, :1380-1413): PL gathered through pl_map, the unseen allele standing in for
 * the alleles mpileup did not see; the Number=R keys through amap.  With --device-alleles bcfgpu_call_constrain does this on the planes */
static void constrained_samples(obuf_t *ob, char **f, const chead_t *h, int S_in)
{
    const int nals = h->nals, unseen = h->unseen; const int *amap = h->amap;
    int pl_map[64], npl = 0;
    for (int i = 0; i < nals; ++i) for (int j = 0; j <= i; ++j) pl_map[npl++] = gt_index(amap[i], amap[j]);
    /* FORMAT keys */
    int nk; char *fmt = strdup(f[8]), **keys = split(fmt, ':', &nk);
    int ipl = -1;
    for (int i = 0; i < nk; ++i) if (!strcmp(keys[i], "PL")) ipl = i;
    if (ipl < 0) DIE("no FORMAT/PL at %s:%s\n", f[0], f[1]);
    /* the widest PL vector of the record is the stride of bcf_get_format_int32 */
    int width = 1;
    char ***sv = malloc((size_t)S_in * sizeof *sv); int *snv = malloc((size_t)S_in * sizeof *snv); char **sc = malloc((size_t)S_in * sizeof *sc);
    for (int s = 0; s < S_in; ++s) {
        sc[s] = strdup(f[9 + s]); sv[s] = split(sc[s], ':', &snv[s]);
        if (ipl < snv[s]) { int w = 1; for (const char *q = sv[s][ipl]; *q; ++q) w += *q == ','; if (w > width) width = w; }
    }
    int32_t *ori = malloc((size_t)width * 4);
    for (int s = 0; s < S_in; ++s) {
        outf(ob, "\t");
        for (int w = 0; w < width; ++w) ori[w] = BCFGPU_INT32_VECTOR_END;
        if (ipl < snv[s]) {
            int np; char *pc = strdup(sv[s][ipl]), **pv = split(pc, ',', &np);
            for (int j = 0; j < np && j < width; ++j) ori[j] = !strcmp(pv[j], ".") ? BCFGPU_INT32_MISSING : atoi(pv[j]);
            free(pv); free(pc);
        } else ori[0] = BCFGPU_INT32_MISSING;
        for (int k = 0; k < nk; ++k) {
            if (k) outf(ob, ":");
            if (k == ipl) {
                int printed = 0;
                for (int g = 0; g < npl; ++g) {
                    int32_t v = pl_map[g] < width ? ori[pl_map[g]] : BCFGPU_INT32_VECTOR_END;
                    if (v == BCFGPU_INT32_MISSING && unseen >= 0) {          /* an allele mpileup did not see: the unseen allele stands in */
                        int ia, ib; gt_alleles(pl_map[g], &ia, &ib);
                        int ko = gt_index(ia, unseen);
                        if ((ko < width ? ori[ko] : BCFGPU_INT32_VECTOR_END) == BCFGPU_INT32_MISSING) ko = gt_index(ib, unseen);
                        if ((ko < width ? ori[ko] : BCFGPU_INT32_VECTOR_END) == BCFGPU_INT32_MISSING) ko = gt_index(unseen, unseen);
                        v = ko < width ? ori[ko] : BCFGPU_INT32_VECTOR_END;
                    }
                    if (g == 0 && v == BCFGPU_INT32_VECTOR_END) v = BCFGPU_INT32_MISSING;
                    if (v == BCFGPU_INT32_VECTOR_END) break;
                    if (printed++) outf(ob, ",");
                    if (v == BCFGPU_INT32_MISSING) outf(ob, "."); else outf(ob, "%d", v);
                }
            } else if (k < snv[s] && is_numberR(fmtR, n_fmtR, keys[k], strlen(keys[k]))) constrained_numberR(ob, sv[s][k], amap, nals);      /* Number=R: new[k] = old[als_map[k]] */
            else outf(ob, "%s", k < snv[s] ? sv[s][k] : ".");
        }
    }
    free(ori);
    for (int s = 0; s < S_in; ++s) { free(sv[s]); free(sc[s]); }
    free(sv); free(snv); free(sc); free(keys); free(fmt);
}
/* The record `line` (n_smp sample columns) in the alleles of target t: a new malloc'ed line, the same line when nothing changes, or
 * NULL when mcall() would return -2 (the site is skipped).  *unseen: in/out.  n_smp is the input's sample count, or 0 with
 * --device-alleles: the line is the first nine columns, the head alone is rewritten, and *kept (when not NULL) takes what the device
 * needs to constrain the planes (amap, the original allele count, the unseen allele before the rewrite, whether anything changes). */
static char *constrain_line(const char *line, const tgt_t *t, int n_smp, int *unseen_io, chead_t *kept)
{
    char *c = strdup(line); int nf; char **f = split(c, '\t', &nf);
    int nalt = 0; char *altc = strdup(f[4]), **alts = split(altc, ',', &nalt);
    if (!strcmp(f[4], ".")) nalt = 0;
    chead_t h; char *res = NULL;
    if (constrain_head(f, alts, nalt, t, *unseen_io, &h) == 0) {
        if (kept) { *kept = h; kept->unseen_al = NULL; }
        if (!h.changed) res = strdup(line);
        else {
            const size_t cap = strlen(line) * 4 + 4096 + (size_t)n_smp * (size_t)(h.nals * (h.nals + 1) / 2) * 12;
            obuf_t ob = { malloc(cap), 0, cap };
            constrained_columns(&ob, f, &h);
            constrained_samples(&ob, f, &h, n_smp);
            *unseen_io = h.unseen ? h.nals - 1 : h.unseen;
            res = ob.p;
        }
    }
    free(h.unseen_al); free(alts); free(altc); free(f); free(c);
    return res;
}

/* next_line (vcfcall.c:501-605): the target of this record, or -1 when the record is not to be called */
static int pick_target(const char *chrom, int pos, const char *ref, char **alts, int nalt)
{
    int best = -1, bestn = 0, any = 0;
    char **als = malloc((size_t)(nalt + 1) * sizeof *als);
    als[0] = (char*)ref; for (int i = 0; i < nalt; ++i) als[1 + i] = alts[i];
    const int rec_indel = als_is_indel(als, nalt + 1) ? 1 : -1;
    for (int x = 0; x < n_tgt; ++x) {
        tgt_t *t = &tgt[tgt_sorted[x]];
        if (strcmp(t->chrom, chrom) || t->pos != pos) continue;
        any = 1;
        if (t->used) continue;
        vcmp_t vc; int n = 0;
        if (vcmp_set_ref(&vc, ref, t->als[0]) == 0) {
            n = 1;
            if (nalt > 0 && t->nals > 1) for (int i = 1; i < t->nals; ++i) n += vcmp_find_allele(&vc, alts, nalt, t->als[i]) >= 0;
        }
        n *= rec_indel * (als_is_indel(t->als, t->nals) ? 1 : -1);
        if (best < 0 || n > bestn) { best = tgt_sorted[x]; bestn = n; }
    }
    free(als);
    (void)any;
    return best;
}

/* ---- -t / -T / -r / -R: the sites to look at, as (sequence, first, last) with 1-based inclusive positions; last < 0: to the end ---- */
typedef struct { char *chrom; long beg, end; } sflt_t;
static sflt_t *sflt; static int n_sflt;
static void site_filter_add(const char *spec)
{
    sflt = realloc(sflt, (size_t)(n_sflt + 1) * sizeof *sflt);
    sflt_t *q = &sflt[n_sflt++];
    const char *c = strrchr(spec, ':');
    q->beg = 1; q->end = -1;
    if (!c) { q->chrom = strdup(spec); return; }
    q->chrom = strndup(spec, (size_t)(c - spec));
    char *e; q->beg = strtol(c + 1, &e, 10);
    if (e == c + 1) { free(q->chrom); q->chrom = strdup(spec); q->beg = 1; return; }      /* a ':' inside the sequence name */
    if (*e == '-') { q->end = e[1] ? strtol(e + 1, NULL, 10) : -1; } else q->end = q->beg;
}
static void site_filter_file(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) DIE("cannot open %s\n", path);
    char ln[4096], c[1024]; long a, b;
    while (fgets(ln, sizeof ln, f)) {
        if (ln[0] == '#') continue;
        const int k = sscanf(ln, "%1023s %ld %ld", c, &a, &b);
        if (k < 1) continue;
        sflt = realloc(sflt, (size_t)(n_sflt + 1) * sizeof *sflt);
        sflt[n_sflt].chrom = strdup(c); sflt[n_sflt].beg = k >= 2 ? a : 1; sflt[n_sflt].end = k >= 3 ? b : k == 2 ? a : -1;
        ++n_sflt;
    }
    fclose(f);
}
static int site_filter_has(const char *line)
{
    const char *t = strchr(line, '\t');
    if (!t) return 0;
    const long pos = atol(t + 1);
    for (int i = 0; i < n_sflt; ++i)
        if (strlen(sflt[i].chrom) == (size_t)(t - line) && !strncmp(sflt[i].chrom, line, (size_t)(t - line)) && pos >= sflt[i].beg && (sflt[i].end < 0 || pos <= sflt[i].end)) return 1;
    return 0;
}

/* the sites `call` passes over before anything else (vcfcall.c:1095-1099): -V snps / indels by htslib's bcf_is_snp (every allele one
 * base that is not '*', or the symbolic <X> / <*>), and -- unless -M -- a reference allele that starts with N */
static int unwanted_site(const char *line, int acgt_only, int skip_kind)
{
    if (n_sflt && !site_filter_has(line)) return 1;
    const char *f = line; int tabs = 0;
    for (; *f && tabs < 3; ++f) if (*f == '\t') ++tabs;
    if (tabs < 3) return 0;
    const char *ref = f, *re = strchr(ref, '\t');
    if (!re) return 0;
    const char *alt = re + 1, *ae = strchr(alt, '\t');
    if (!ae) ae = alt + strlen(alt);
    if (skip_kind) {
        int is_snp = (re - ref == 1 && ref[0] != '*');
        if (!(ae - alt == 1 && alt[0] == '.'))
            for (const char *a = alt; is_snp && a < ae; ) {
                const char *e = memchr(a, ',', (size_t)(ae - a)); if (!e) e = ae;
                const size_t l = (size_t)(e - a);
                if (!((l == 1 && a[0] != '*') || (l == 3 && a[0] == '<' && (a[1] == 'X' || a[1] == '*') && a[2] == '>'))) is_snp = 0;
                a = e + 1;
            }
        if (skip_kind == 1 && is_snp) return 1;                  /* -V snps: CF_INDEL_ONLY */
        if (skip_kind == 2 && !is_snp) return 1;                 /* -V indels: CF_NO_INDEL */
    }
    return acgt_only && (ref[0] == 'N' || ref[0] == 'n');
}


/* ---- the state of a run, stage by stage ---- */
typedef struct {                                                /* the command line */
    int varonly, out_tags, keepalt, dev_in, dev_parse, parse_given, dev_rec, dev_keys, keys_given, dev_text, text_given, dev_als, als_given, want_timing;
    int acgt_only, skip_kind;                                   /* vcfcall.c:937 (CF_ACGT_ONLY is the default); -V: 1 = snps, 2 = indels */
    const char *tgt_file, *smpl_file, *smpl_list, *ploidy_file, *ploidy_alias, *grp_arg, *grp_tag, *out_path, *in_path;
    double prior; char out_mode, prior_an_tag[64], prior_ac_tag[64];
    int32_t gv_range[16]; int gv_n;                             /* -g INT,...: gvcf_init (gvcf.c:47-73) */
} opt_t;
/* ploidy definition (ploidy.c): regions per sex, '*' lines = the sex's default; the last sex named is the default sex;
 * max: ploidy_max() of the definition -- the prior counts max * samples alleles (vcfcall.c:652-656, mcall.c:396-416) */
typedef struct { preg_t *reg; int n, max; char last_sex[64]; } ploidy_t;
/* the samples called, S of the input's S_in: output sample s = input column col[s] (bcf_subset with -S); the names of the input
 * columns; a sample's ploidy ("0", "1", "2") or sex name; -G: the group of every sample */
typedef struct { int S, S_in, *col; char **names, (*spec)[64]; int32_t *grp; int ngrp; } smap_t;
/* the records that are called; --device-input: their per-sample blocks, back to back (--device-parse: their sample columns' text); -i: where the last record lay */
typedef struct { rec_t *rec; int n, cap, ngmax, namax; unsigned char *ibuf; size_t ibuf_l, ibuf_m; char *prev_chrom; long prev_pos0;
                 int ngin, nain, n_changed; } recs_t;           /* --device-alleles: the genotypes / alleles of the widest input record; the records -C alleles changes */
/* what mcall() reads from the records: PL planes (missing / vector_end kept), QS, I16.
 * --device-input: no host PL / AD planes; per record where the PL vector (and the -G tag's) lies in the byte buffer.
 * --device-parse: likewise; per record where its columns lie in the byte buffer and the key's place in the FORMAT column */
typedef struct { int32_t *nals, *unseen, *pl, *ad, *pan, *pac; float *qs, *i16; bcfgpu_bcf_vec *vec_pl, *vec_ad; bcfgpu_vcf_vec *txt_pl, *txt_ad; int want_ad; } hplanes_t;
typedef struct {                                                /* the planes in HBM, and what came down of the results */
    bcfgpu_ctx *ctx;
    int32_t *d_nals, *d_unseen, *d_plin, *d_ad, *d_grp, *d_pan, *d_pac; float *d_qs, *d_i16;
    void *d_indiv;                                              /* --device-keys, --device-text: the input's bytes or text, kept until the pass-through keys / the columns are made */
    void *d_site, *d_gt, *d_pl, *d_ploidy, *d_gq, *d_gp;
    bcfgpu_call_site *cs; int8_t *gt; int32_t *opl, *gq; float *gp;
} dev_t;
typedef struct {                                                /* --device-records, --device-keys: the blocks made in HBM */
    uint8_t *emit; void *d_emit;                                /* which records are written */
    unsigned char *kblk; uint64_t *koff; int n_enc;
    unsigned char *pblk; uint64_t *poff; long n_pjob, n_phost;  /* --device-keys: the pass-through keys' blocks, one offset a job */
    unsigned char *tblk; uint64_t *toff; long n_tdev, n_thost;  /* --device-text: the sample columns as text, one offset a record (equal: the host's) */
} blocks_t;
typedef struct { int32_t *w, *blk, *min, *dp; bcfgpu_gvcf_block *block; } gvcf_t;   /* -g: record k is written record w[k], or -1 */
static void gvcf_option(opt_t *o, const char *arg, const char *echo) { if ((o->gv_n = parse_gvcf_limits(arg, o->gv_range)) < 0) DIE("Could not parse: --gvcf %s\n", echo); }
/* 0, or 2 after the usage text */
static int parse_options(int argc, char **argv, opt_t *o)
{
    {   /* call's long option names (vcfcall.c:946-981) are read as their short forms; -f is the old spelling of -a (vcfcall.c:995) */
        static const char *alias[][2] = {
            { "--variants-only", "-v" }, { "--multiallelic-caller", "-m" }, { "--keep-alts", "-A" }, { "--insert-missed", "-i" }, { "--constrain", "-C" },
            { "--targets-file", "-T" }, { "--prior", "-P" }, { "--output-type", "-O" }, { "--output", "-o" }, { "--group-samples", "-G" },
            { "--prior-freqs", "-F" }, { "--annotate", "-a" }, { "--format-fields", "-a" }, { "-f", "-a" }, { "--samples-file", "-S" }, { "--samples", "-s" },
            { "--pval-threshold", "-p" } };
        for (int i = 1; i < argc; ++i)
            for (size_t k = 0; k < sizeof alias / sizeof alias[0]; ++k) if (!strcmp(argv[i], alias[k][0])) argv[i] = (char *)alias[k][1];
    }
    memset(o, 0, sizeof *o); o->acgt_only = 1; o->prior = 1.1e-3; o->out_mode = 'v'; o->out_path = "-";
    while (argc > 2 && argv[1][0] == '-') {
        if (!strcmp(argv[1], "-v")) { o->varonly = 1; ++argv; --argc; }
        else if (!strcmp(argv[1], "-m")) { ++argv; --argc; }                                     /* the multiallelic caller: the only one here */
        else if (!strcmp(argv[1], "-A")) { o->keepalt = 1; ++argv; --argc; }
        else if (!strcmp(argv[1], "-M") || !strcmp(argv[1], "--keep-masked-refs")) { o->acgt_only = 0; ++argv; --argc; }      /* vcfcall.c:1000 */
        else if (!strcmp(argv[1], "-N") || !strcmp(argv[1], "--skip-Ns")) { o->acgt_only = 1; ++argv; --argc; }               /* vcfcall.c:1001: the default */
        else if ((!strcmp(argv[1], "-V") || !strcmp(argv[1], "--skip-variants")) && argc > 3) {                              /* vcfcall.c:1032-1036 */
            if (!strcasecmp(argv[2], "snps")) o->skip_kind = 1; else if (!strcasecmp(argv[2], "indels")) o->skip_kind = 2;
            else DIE("Unknown skip category \"%s\" (-V argument must be \"snps\" or \"indels\")\n", argv[2]);
            argv += 2; argc -= 2;
        }
        else if (!strcmp(argv[1], "--threads") && argc > 3) { argv += 2; argc -= 2; }                                        /* (compression threads: nothing to do here) */
        else if (!strcmp(argv[1], "--no-version")) { ++argv; --argc; }                                                       /* (no ##bcftools_callVersion lines are written anyway) */
        else if (!strcmp(argv[1], "-i")) { insert_missed = 1; ++argv; --argc; }
        else if (!strcmp(argv[1], "--device-input")) { o->dev_in = 1; ++argv; --argc; }
        else if (!strcmp(argv[1], "--device-parse")) { o->dev_parse = o->parse_given = 1; ++argv; --argc; }
        else if (!strcmp(argv[1], "--device-records")) { o->dev_rec = 1; ++argv; --argc; }
        else if (!strcmp(argv[1], "--device-keys")) { o->dev_keys = o->keys_given = 1; ++argv; --argc; }
        else if (!strcmp(argv[1], "--device-text")) { o->dev_text = o->text_given = 1; ++argv; --argc; }
        else if (!strcmp(argv[1], "--device-alleles")) { o->dev_als = o->als_given = 1; ++argv; --argc; }
        else if (!strcmp(argv[1], "--timing")) { o->want_timing = 1; ++argv; --argc; }
        else if (!strcmp(argv[1], "-C") && argc > 3) { if (strcmp(argv[2], "alleles")) DIE("-C: only `alleles` is supported\n"); cals = 1; argv += 2; argc -= 2; }
        else if (!strcmp(argv[1], "-T") && argc > 3) { o->tgt_file = argv[2]; argv += 2; argc -= 2; }
        else if ((!strcmp(argv[1], "-t") || !strcmp(argv[1], "--targets") || !strcmp(argv[1], "-r") || !strcmp(argv[1], "--regions")) && argc > 3) {
            /* -t / -r CHR[:POS | :BEG-END],...: only the records whose POS lies there (bcf_sr_set_targets / _regions, vcfcall.c:612-626; -r without
             * an index is a filter over the stream here) */
            char *c = strdup(argv[2]); int nt; char **t = split(c, ',', &nt);
            for (int i = 0; i < nt; ++i) site_filter_add(t[i]);
            free(t); free(c); argv += 2; argc -= 2;
        }
        else if ((!strcmp(argv[1], "-R") || !strcmp(argv[1], "--regions-file")) && argc > 3) { site_filter_file(argv[2]); argv += 2; argc -= 2; }
        else if (!strcmp(argv[1], "-P") && argc > 3) { o->prior = atof(argv[2]); argv += 2; argc -= 2; }      /* vcfcall.c:931-943 */
        else if (!strcmp(argv[1], "-O") && argc > 3) { o->out_mode = argv[2][0]; argv += 2; argc -= 2; }      /* version.c:67-82 */
        else if (!strncmp(argv[1], "-O", 2) && argv[1][2]) { o->out_mode = argv[1][2]; ++argv; --argc; }
        else if (!strcmp(argv[1], "-o") && argc > 3) { o->out_path = argv[2]; argv += 2; argc -= 2; }
        else if (!strcmp(argv[1], "-G") && argc > 3) { o->grp_arg = argv[2]; argv += 2; argc -= 2; }
        else if (!strcmp(argv[1], "--group-samples-tag") && argc > 3) { o->grp_tag = argv[2]; argv += 2; argc -= 2; }
        else if (!strcmp(argv[1], "-F") && argc > 3) {
            const char *c = strchr(argv[2], ',');
            if (!c || c == argv[2] || !c[1] || c - argv[2] > 63 || strlen(c + 1) > 63) DIE("-F: expected AN_TAG,AC_TAG\n");
            memcpy(o->prior_an_tag, argv[2], (size_t)(c - argv[2])); o->prior_an_tag[c - argv[2]] = 0; strcpy(o->prior_ac_tag, c + 1);
            argv += 2; argc -= 2;
        }
        else if (!strcmp(argv[1], "-a") && argc > 3) {
            char *c = strdup(argv[2]); int nt; char **t = split(c, ',', &nt);
            for (int i = 0; i < nt; ++i)
                if (!strcmp(t[i], "GQ")) o->out_tags |= BCFGPU_CALL_FMT_GQ;
                else if (!strcmp(t[i], "GP")) o->out_tags |= BCFGPU_CALL_FMT_GP;
                else DIE("-a: unknown tag %s\n", t[i]);
            free(t); free(c); argv += 2; argc -= 2;
        }
        else if ((!strcmp(argv[1], "-g") || !strcmp(argv[1], "--gvcf")) && argc > 3) { gvcf_option(o, argv[2], argv[2]); argv += 2; argc -= 2; }
        else if ((!strncmp(argv[1], "-g", 2) && argv[1][2]) || (!strncmp(argv[1], "-mg", 3) && argv[1][3])) {   /* -g0,2,5; the `-mg0` of test.pl:277 */
            gvcf_option(o, argv[1] + (argv[1][1] == 'm' ? 3 : 2), argv[1] + 2); ++argv; --argc;
        }
        else if (!strcmp(argv[1], "-S") && argc > 3) { o->smpl_file = argv[2]; argv += 2; argc -= 2; }
        else if (!strcmp(argv[1], "-s") && argc > 3) { o->smpl_list = argv[2]; o->smpl_file = argv[2]; argv += 2; argc -= 2; }          /* -s LIST: the names, comma-separated (vcfcall.c:1050) */
        else if (!strcmp(argv[1], "-p") && argc > 3) { argv += 2; argc -= 2; }                                                 /* --pval-threshold: read by the consensus caller only (vcfcall.c:1038) */
        else if (!strcmp(argv[1], "--ploidy-file") && argc > 3) { o->ploidy_file = argv[2]; argv += 2; argc -= 2; }
        else if (!strcmp(argv[1], "--ploidy") && argc > 3) { o->ploidy_alias = argv[2]; argv += 2; argc -= 2; }                       /* vcfcall.c:976, 827-855 */
        else if (!strcmp(argv[1], "-X")) { o->ploidy_alias = "X"; ++argv; --argc; }                                                  /* vcfcall.c:991 */
        else if (!strcmp(argv[1], "-Y")) { o->ploidy_alias = "Y"; ++argv; --argc; }                                                  /* vcfcall.c:992 */
        else break;
    }
    if (o->gv_n && o->varonly) DIE("The two options cannot be combined: --variants-only and --gvcf\n");       /* vcfcall.c:1085 */
    if (o->gv_n && cals) DIE("-g with -C alleles is not supported\n");
    if (argc != 2) { fprintf(stderr, "usage: bcfgpu_call [-v] [-M] [-V snps|indels] [-t|-r REGIONS] [-T|-R FILE] [-g INT,...] [-S samples.txt | -s NAME,...] [--ploidy-file file | --ploidy GRCh37|GRCh38|X|Y|1] [-G -|groups.txt [--group-samples-tag TAG]] [-F AN,AC] [-a GQ,GP] [-A] [-P theta] [-C alleles -T targets.tab [-i]] [--device-input] [--device-parse] [--device-alleles] [--device-records] [--device-keys] [--device-text] [--timing] [-O v|z|u|b] [-o out] in.vcf|in.bcf\n"
        "       --device-alleles acts with -C alleles where --device-input (BCF in) or --device-parse (VCF text in) is given: that option then takes effect\n"
        "       --device-text acts with -O v|z where --device-input (BCF in) or --device-parse (VCF text in) is in effect\n"
        "       --device-keys acts with -O u|b where --device-records and --device-input (BCF in) or --device-parse (VCF text in) are in effect\n"); return 2; }
    o->in_path = argv[1]; return 0;
}
static void load_ploidy(opt_t *o, ploidy_t *P)
{
    memset(P, 0, sizeof *P); char *alias_text = NULL;
    P->max = 2;                                                  /* no definition given: `0 0 / 1 1 / 2 2` (vcfcall.c:1071) */
    if (o->ploidy_alias) {
        /* --ploidy ALIAS: the definitions `call` carries with it (vcfcall.c:138-199), in the format of a --ploidy-file: the
         * haploid stretches of the human sex chromosomes outside the pseudo-autosomal regions and the mitochondrion, by assembly;
         * "X" / "Y" / "1": males haploid / males haploid and females absent / everybody haploid, whatever the sequence */
        static const struct { const char *name; long x_par1_end, x_par2_beg, x_end, y_end; } asm_[2] = {
            { "GRCh37", 60000, 2699521, 154931043, 59373566 }, { "GRCh38", 9999, 2781480, 155701381, 57227415 } };
        size_t al = 0; FILE *m = open_memstream(&alias_text, &al); int known = 0;
        for (int k = 0; k < 2; ++k)
            if (!strcmp(o->ploidy_alias, asm_[k].name)) {
                for (int pre = 0; pre < 2; ++pre) {
                    const char *c = pre ? "chr" : "";
                    fprintf(m, "%sX 1 %ld M 1\n%sX %ld %ld M 1\n%sY 1 %ld M 1\n%sY 1 %ld F 0\n", c, asm_[k].x_par1_end, c, asm_[k].x_par2_beg, asm_[k].x_end, c, asm_[k].y_end, c, asm_[k].y_end);
                    fprintf(m, "%s 1 16569 M 1\n%s 1 16569 F 1\n", pre ? "chrM" : "MT", pre ? "chrM" : "MT");
                }
                fprintf(m, "* * * M 2\n* * * F 2\n");
                known = 1;
            }
        if (!strcmp(o->ploidy_alias, "X")) { fprintf(m, "* * * M 1\n* * * F 2\n"); known = 1; }
        if (!strcmp(o->ploidy_alias, "Y")) { fprintf(m, "* * * M 1\n* * * F 0\n"); known = 1; }
        if (!strcmp(o->ploidy_alias, "1")) { fprintf(m, "* * * * 1\n"); known = 1; }
        fclose(m);
        if (!known) DIE("--ploidy: GRCh37, GRCh38, X, Y or 1 (or a --ploidy-file)\n");
        if (o->ploidy_file) DIE("--ploidy and --ploidy-file exclude each other\n");
        o->ploidy_file = "--ploidy";
    }
    if (!o->ploidy_file) return;
    FILE *pf = alias_text ? fmemopen(alias_text, strlen(alias_text), "r") : fopen(o->ploidy_file, "r");
    if (!pf) DIE("cannot open %s\n", o->ploidy_file);
    char ln[1024], c[256], a[64], b[64], sx[64]; int pl;
    while (fgets(ln, sizeof ln, pf))
        if (sscanf(ln, "%255s %63s %63s %63s %d", c, a, b, sx, &pl) == 5) {
            P->reg = realloc(P->reg, (size_t)(P->n + 1) * sizeof *P->reg);
            preg_t *q = &P->reg[P->n++];
            strcpy(q->chrom, c); strcpy(q->sex, sx); q->ploidy = pl;
            q->from = !strcmp(a, "*") ? -1 : atoi(a); q->to = !strcmp(b, "*") ? -1 : atoi(b);
            strcpy(P->last_sex, sx);
        }
    fclose(pf);
    /* ploidy_max() (ploidy.c:109-110, 122-131, 259-262): the largest ploidy of any line, default lines included, or the definition's
     * own default if that is larger -- the default of the sex named "*" where the definition has one, else 2.  So `* * * * 1` alone
     * gives 1, `* * * M 1` with `* * * F 1` gives 2.  (Not reproduced: a region line of the sex "*" without a `* * * *` line, which
     * leaves the reference's default at -1.) */
    int dflt = 2, max = -1;
    for (int i = 0; i < P->n; ++i) {
        if (P->reg[i].ploidy > max) max = P->reg[i].ploidy;
        if (P->reg[i].from < 0 && !strcmp(P->reg[i].chrom, "*") && !strcmp(P->reg[i].sex, "*")) dflt = P->reg[i].ploidy;
    }
    P->max = dflt > max ? dflt : max;
}
/* the input and its header; which of the device options take effect in this run */
static vio_file *open_input(opt_t *o, vio_hdr **hdr)
{
    vio_file *fin = vio_open_read(o->in_path);               /* VCF, bgzipped VCF or BCF (hts_open of vcfcall.c) */
    if (!fin) DIE("%s\n", vio_error());
    if (!(*hdr = vio_read_hdr(fin))) DIE("%s\n", vio_error());
    o->dev_in = o->dev_in && vio_is_bcf(fin) && (!cals || o->dev_als) && !o->gv_n;      /* -C alleles rewrites a record's PL, -g reads every record's DP: on the host */
    o->dev_parse = o->dev_parse && !vio_is_bcf(fin) && (!cals || o->dev_als) && !o->gv_n;   /* the same two, for the same reasons, on text input */
    o->dev_als = o->dev_als && cals && (o->dev_in || o->dev_parse);     /* ... unless --device-alleles has the device constrain the planes it decodes */
    o->dev_rec = o->dev_rec && (o->out_mode == 'u' || o->out_mode == 'b') && !o->gv_n;    /* key blocks go into BCF records; -g's block lines read gt on the host */
    o->dev_keys = o->dev_keys && (o->dev_in || o->dev_parse) && o->dev_rec;      /* the input's bytes or text in HBM and key blocks to splice: both ends on the device */
    o->dev_text = o->dev_text && (o->dev_in || o->dev_parse) && (o->out_mode == 'v' || o->out_mode == 'z');   /* the input's bytes or text in HBM, text records to write */
    return fin;
}
/* the samples of the header, or those of -S / -s in that order (vcfcall.c:202-344) */
static void map_samples(const opt_t *o, const ploidy_t *P, const vio_hdr *hdr, smap_t *M)
{
    memset(M, 0, sizeof *M); M->ngrp = 1;
    const int S_in = M->S_in = M->S = vio_hdr_nsamples(hdr);
    M->names = malloc((size_t)(S_in > 0 ? S_in : 1) * sizeof *M->names);
    for (int s = 0; s < S_in; ++s) M->names[s] = strdup(vio_hdr_sample(hdr, s));
    M->col = malloc((size_t)(S_in > 0 ? S_in : 1) * sizeof *M->col);
    M->spec = malloc((size_t)(S_in > 0 ? S_in : 1) * sizeof *M->spec);
    for (int s = 0; s < S_in; ++s) { M->col[s] = s; strcpy(M->spec[s], o->ploidy_file ? P->last_sex : "2"); }   /* vcfcall.c:645-650 */
    if (!o->smpl_file) return;
    char *lbuf = NULL;
    if (o->smpl_list) { lbuf = strdup(o->smpl_list); for (char *c = lbuf; *c; ++c) if (*c == ',') *c = '\n'; }
    FILE *sf = o->smpl_list ? fmemopen(lbuf, strlen(lbuf), "r") : fopen(o->smpl_file, "r");
    if (!sf) DIE("cannot open %s\n", o->smpl_file);
    char ln[1024]; int m = 0;
    while (fgets(ln, sizeof ln, sf)) {
        char w[6][256]; const int nw = sscanf(ln, "%255s %255s %255s %255s %255s %255s", w[0], w[1], w[2], w[3], w[4], w[5]);
        if (nw < 1 || w[0][0] == '#') continue;
        const char *name = nw >= 5 ? w[1] : w[0];                   /* PED: family, sample, father, mother, sex */
        const char *sp = nw >= 5 ? (!strcmp(w[4], "1") ? "M" : "F") : nw >= 2 ? w[1] : "2";
        int i;
        for (i = 0; i < S_in; ++i) if (!strcmp(M->names[i], name)) break;
        if (i == S_in) continue;                                    /* not in the VCF: ignored */
        if (m == S_in) DIE("too many samples in %s\n", o->smpl_file);
        M->col[m] = i; strcpy(M->spec[m], sp); ++m;
    }
    fclose(sf); free(lbuf); M->S = m;
}
/* the unseen allele as vcfcall.c:1102-1111 finds it: 1 + the index of the first ALT that is X, <X> or <*>, or 0 */
static int unseen_allele(char **alts, int nalt)
{
    for (int i = 0; i < nalt; ++i) { const char *a = alts[i]; if (a[0] == 'X' || (a[0] == '<' && (a[1] == 'X' || a[1] == '*') && a[2] == '>')) return 1 + i; }
    return 0;
}
/* -C alleles: pair the record with a target, rewrite it.  The line to call (malloc'ed), or NULL: the record is passed over.
 * --device-alleles: buf is the first nine columns (n_smp = 0), the head alone is rewritten and *kept says how the planes follow */
static char *pair_with_target(const opt_t *o, const char *buf, int n_smp, recs_t *R, chead_t *kept)
{
    char *owned = NULL, *c2 = strdup(buf); int nf2; char **f2 = split(c2, '\t', &nf2);
    if (nf2 != 9 + n_smp) DIE("malformed VCF\n");
    int nalt2 = 0; char *ac = strdup(f2[4]), **av = split(ac, ',', &nalt2);
    if (!strcmp(f2[4], ".")) nalt2 = 0;
    const int pos2 = atoi(f2[1]), ti = pick_target(f2[0], pos2, f2[3], av, nalt2);
    if (ti >= 0) {
        tgt[ti].used = 1; int un = unseen_allele(av, nalt2);
        owned = constrain_line(buf, &tgt[ti], n_smp, &un, kept);
        if (owned && unwanted_site(owned, o->acgt_only, o->skip_kind)) { free(owned); owned = NULL; }   /* (the skipped record flushes no targets either: vcfcall.c:1095-1099 come before tgt_flush) */
        if (owned && insert_missed) {                    /* tgt_flush (vcfcall.c:426-455) */
            const long p0 = pos2 - 1;
            if (!R->prev_chrom) flush_region(f2[0], 0, p0 - 1);
            else if (strcmp(R->prev_chrom, f2[0])) { flush_region(R->prev_chrom, R->prev_pos0 + 1, 1L << 40); flush_region(f2[0], 0, p0 - 1); }
            else flush_region(R->prev_chrom, R->prev_pos0, p0 - 1);
            free(R->prev_chrom); R->prev_chrom = strdup(f2[0]); R->prev_pos0 = p0;
        }
    }
    free(av); free(ac); free(f2); free(c2);
    return owned;
}
/* alleles; the unseen allele */
static void record_alleles(rec_t *r)
{
    int nalt = 0; char *alt = strdup(r->fld[4]), **alts = split(alt, ',', &nalt);
    if (!strcmp(r->fld[4], ".")) nalt = 0;
    r->nals = 1 + nalt; r->als = malloc((size_t)r->nals * sizeof *r->als); r->als[0] = r->fld[3];
    for (int i = 0; i < nalt; ++i) r->als[1 + i] = alts[i];
    r->unseen = unseen_allele(alts, nalt);
    free(alts);
    if (r->nals > 5) DIE("more than 5 alleles at %s:%s\n", r->fld[0], r->fld[1]);
}
/* the ploidy of every sample at this record (set_ploidy, vcfcall.c:807-825) */
static void record_ploidy(rec_t *r, const ploidy_t *P, const smap_t *M)
{
    const preg_t *preg = P->reg; const int npreg = P->n, S = M->S, pos1 = atoi(r->fld[1]);
    uint8_t *ploidy = r->ploidy = malloc((size_t)S);
    for (int s = 0; s < S; ++s) {
        const char *spec = M->spec[s]; int pl = 2;
        if (!strcmp(spec, "0") || !strcmp(spec, "1") || !strcmp(spec, "2")) pl = atoi(spec);
        else {
            int found = 0;
            for (int i = 0; i < npreg && !found; ++i)
                if (preg[i].from >= 0 && !strcmp(preg[i].chrom, r->fld[0]) && !strcmp(preg[i].sex, spec) && preg[i].from <= pos1 && pos1 <= preg[i].to) { pl = preg[i].ploidy; found = 1; }
            for (int i = 0; i < npreg && !found; ++i)
                if (preg[i].from < 0 && !strcmp(preg[i].sex, spec)) { pl = preg[i].ploidy; found = 1; }
            for (int i = 0; i < npreg && !found; ++i)                       /* a sex without a default of its own takes the "*" sex's (ploidy.c:122-127) */
                if (preg[i].from < 0 && !strcmp(preg[i].sex, "*")) { pl = preg[i].ploidy; found = 1; }
        }
        ploidy[s] = (uint8_t)pl;
    }
}
/* the read loop: the records that are called, split into fields; closes the input */
static void read_records(const opt_t *o, const ploidy_t *P, const smap_t *M, vio_file *fin, vio_hdr *hdr, recs_t *R)
{
    memset(R, 0, sizeof *R); R->ngmax = R->ngin = R->nain = 1;
    const int S_in = M->S_in;
    char *buf = NULL; size_t bufcap = 0; int rrc;
    if (cals) { if (!o->tgt_file) DIE("-C alleles needs -T targets\n"); tgt_parse(o->tgt_file); }
    else if (o->tgt_file) site_filter_file(o->tgt_file);     /* -T without -C alleles: the targets restrict the sites (vcfcall.c:612-617) */
    for (;;) {
        const void *indiv = NULL; size_t l_indiv = 0; int n_fmt = 0, n_sample = 0;
        rrc = o->dev_in ? vio_read_record(fin, hdr, &buf, &bufcap, &indiv, &l_indiv, &n_fmt, &n_sample) : vio_read_line(fin, hdr, &buf, &bufcap);
        if (rrc <= 0) break;
        if (!strlen(buf)) continue;
        char *use = buf, *owned = NULL;
        const char *smp = NULL;                                  /* --device-parse: the ninth tab, where the sample columns start */
        if (o->dev_parse) {
            smp = buf;
            for (int t = 0; t < 9 && smp; ++t) smp = strchr(smp + (t > 0), '\t');
            if (!smp) DIE("malformed VCF\n");
        }
        chead_t kept; memset(&kept, 0, sizeof kept);
        if (cals && o->dev_als) {                                /* the head alone is paired and rewritten; the samples' bytes or text stay as they are */
            char *head = smp ? strndup(buf, (size_t)(smp - buf)) : buf;
            use = owned = pair_with_target(o, head, 0, R, &kept);
            if (smp) free(head);
            if (!use) continue;
        }
        else if (cals) { if (!(use = owned = pair_with_target(o, buf, S_in, R, NULL))) continue; }
        else if (unwanted_site(use, o->acgt_only, o->skip_kind)) continue;
        if (R->n == R->cap) { R->cap = R->cap ? 2 * R->cap : 1024; R->rec = realloc(R->rec, (size_t)R->cap * sizeof *R->rec); }
        if (cals) push_event(0, R->n);
        rec_t *r = &R->rec[R->n++];
        r->line = smp && !o->dev_als ? strndup(use, (size_t)(smp - use)) : strdup(use);
        r->fld = split(r->line, '\t', &r->nfld);
        r->keys = NULL; r->nkeys = 0; r->kjob = NULL; r->nkjob = 0;
        r->nori = kept.nori; r->unseen_in = kept.unseen; r->changed = kept.changed;
        for (int i = 0; i < BCFGPU_MAX_ALLELES; ++i) r->amap[i] = i < kept.nals ? kept.amap[i] : 0;
        if (o->dev_als) { R->n_changed += r->changed; if (r->nori * (r->nori + 1) / 2 > R->ngin) R->ngin = r->nori * (r->nori + 1) / 2; if (r->nori > R->nain) R->nain = r->nori; }
        if (smp) {                                               /* the columns join the byte buffer as they are */
            const size_t l_smp = strlen(smp);
            if (R->ibuf_l + l_smp > R->ibuf_m) { R->ibuf_m = (R->ibuf_l + l_smp) * 2 + (1 << 20); R->ibuf = realloc(R->ibuf, R->ibuf_m); if (!R->ibuf) DIE("out of memory\n"); }
            memcpy(R->ibuf + R->ibuf_l, smp, l_smp);
            r->ioff = R->ibuf_l; r->ilen = l_smp; R->ibuf_l += l_smp;
            if (l_smp > UINT32_MAX) DIE("malformed VCF\n");
        }
        free(owned);
        if (o->dev_in) {                                         /* the block joins the byte buffer; where its keys' values lie */
            if (r->nfld != 9 || n_sample != S_in) DIE("malformed VCF\n");
            if (R->ibuf_l + l_indiv > R->ibuf_m) { R->ibuf_m = (R->ibuf_l + l_indiv) * 2 + (1 << 20); R->ibuf = realloc(R->ibuf, R->ibuf_m); if (!R->ibuf) DIE("out of memory\n"); }
            memcpy(R->ibuf + R->ibuf_l, indiv, l_indiv);
            r->ioff = R->ibuf_l; r->ilen = l_indiv; r->n_fmt = n_fmt; R->ibuf_l += l_indiv;
            r->keys = malloc((size_t)(n_fmt > 0 ? (n_fmt < 64 ? n_fmt : 64) : 1) * sizeof *r->keys);
            if ((r->nkeys = vio_indiv_keys(hdr, indiv, l_indiv, n_fmt, n_sample, r->keys)) < 0) DIE("%s\n", vio_error());
        } else
        if (S_in < 0 || r->nfld != (smp ? 9 : 9 + S_in)) DIE("malformed VCF\n");     /* (--device-parse: the device counts the columns) */
        record_alleles(r); record_ploidy(r, P, M);
        if (r->nals * (r->nals + 1) / 2 > R->ngmax) R->ngmax = r->nals * (r->nals + 1) / 2;
    }
    if (rrc < 0) DIE("%s\n", vio_error());
    vio_close(fin);
}
/* -i: the targets behind the last record, then the sequences without any */
static void flush_last_targets(const recs_t *R)
{
    if (!cals || !insert_missed) return;
    if (R->prev_chrom) flush_region(R->prev_chrom, R->prev_pos0, 1L << 40);
    for (int x = 0; x < n_tgt; ++x) if (!tgt[tgt_sorted[x]].used) flush_region(tgt[tgt_sorted[x]].chrom, 0, 1L << 40);
}

/* ---- -G: the group of every sample; ids in the order the groups first appear in the file (mcall.c:308-330) ---- */
static void read_groups(opt_t *o, smap_t *M)
{
    const int S = M->S;
    if (o->grp_arg && !strcmp(o->grp_arg, "-")) {
        M->grp = malloc((size_t)S * 4); M->ngrp = S;
        for (int s = 0; s < S; ++s) M->grp[s] = s;
    } else if (o->grp_arg) {
        FILE *gf = fopen(o->grp_arg, "r");
        if (!gf) DIE("cannot open %s\n", o->grp_arg);
        M->grp = malloc((size_t)S * 4);
        for (int s = 0; s < S; ++s) M->grp[s] = -1;
        char (*gname)[256] = NULL; char ln[1024], w0[256], w1[256]; int ngrp = 0;
        while (fgets(ln, sizeof ln, gf)) {
            if (sscanf(ln, "%255s %255s", w0, w1) != 2 || w0[0] == '#') continue;
            int s, g;
            for (s = 0; s < S; ++s) if (!strcmp(M->names[M->col[s]], w0)) break;
            if (s == S) continue;                                           /* not among the samples called */
            for (g = 0; g < ngrp; ++g) if (!strcmp(gname[g], w1)) break;
            if (g == ngrp) { gname = realloc(gname, (size_t)(ngrp + 1) * sizeof *gname); strcpy(gname[ngrp++], w1); }
            M->grp[s] = g;
        }
        fclose(gf); free(gname);
        M->ngrp = ngrp;
        for (int s = 0; s < S; ++s) if (M->grp[s] < 0) DIE("sample %s is in no group of %s\n", M->names[M->col[s]], o->grp_arg);
    }
    if (M->ngrp > 1 && !o->grp_tag) o->grp_tag = has_fmt_qs ? "QS" : has_fmt_ad ? "AD" : NULL;       /* mcall.c:272-281 */
    if (M->ngrp > 1 && !o->grp_tag) DIE("-G needs FORMAT/QS or FORMAT/AD\n");
}

/* ---- what mcall() reads from the records ---- */
/* FORMAT/PL and the -G tag among the record's keys; --device-input: where their vectors lie in the byte buffer; --device-parse: the
 * record's columns and the keys' places */
static void format_lookup(const opt_t *o, rec_t *r, int want_ad, bcfgpu_bcf_vec *vec_pl, bcfgpu_bcf_vec *vec_ad, bcfgpu_vcf_vec *txt_pl, bcfgpu_vcf_vec *txt_ad)
{
    r->pl_idx = r->ad_idx = -1;
    int nk = r->nkeys; char *fmt = NULL, **keys = NULL;          /* the keys' names: the block's, or the FORMAT column's */
    if (!o->dev_in) { fmt = strdup(r->fld[8]); keys = split(fmt, ':', &nk); }
    for (int i = 0; i < nk; ++i) {
        const char *id = keys ? keys[i] : r->keys[i].id;
        if (!strcmp(id, "PL")) r->pl_idx = i;
        if (want_ad && !strcmp(id, o->grp_tag)) r->ad_idx = i;
    }
    free(keys); free(fmt);
    if (r->pl_idx < 0) DIE("no FORMAT/PL at %s:%s\n", r->fld[0], r->fld[1]);
    if (want_ad && r->ad_idx < 0) DIE("FORMAT/%s is required with -G (%s:%s)\n", o->grp_tag, r->fld[0], r->fld[1]);     /* mcall.c:1476 */
    if (txt_pl) { txt_pl->off = r->ioff; txt_pl->len = (uint32_t)r->ilen; txt_pl->idx = r->pl_idx; }
    if (txt_ad) { *txt_ad = *txt_pl; txt_ad->idx = r->ad_idx; }
    if (!o->dev_in) return;
    const vio_indiv_key *kp = &r->keys[r->pl_idx], *ka = want_ad ? &r->keys[r->ad_idx] : NULL;
    if (kp->type < 1 || kp->type > 3) DIE("FORMAT/PL is not an integer vector at %s:%s\n", r->fld[0], r->fld[1]);
    if (ka && (ka->type < 1 || ka->type > 3)) DIE("FORMAT/%s is not an integer vector at %s:%s\n", o->grp_tag, r->fld[0], r->fld[1]);
    vec_pl->off = r->ioff + kp->off; vec_pl->type = kp->type; vec_pl->width = kp->width;
    if (ka) { vec_ad->off = r->ioff + ka->off; vec_ad->type = ka->type; vec_ad->width = ka->width; }
}
/* a sample's value list of key `idx` into column s of a [width][S] plane; without the key the first value is missing */
static void parse_int_list(char **vals, int nv, int idx, int32_t *plane, int width, int S, int s)
{
    if (idx < nv) {
        int np; char **pv = split(vals[idx], ',', &np);
        for (int j = 0; j < np && j < width; ++j) plane[(size_t)j * S + s] = !strcmp(pv[j], ".") ? BCFGPU_INT32_MISSING : atoi(pv[j]);
        free(pv);
    } else plane[s] = BCFGPU_INT32_MISSING;
}
/* INFO/QS, INFO/I16 and the -F tags of record k */
static void parse_info(const opt_t *o, const rec_t *r, hplanes_t *H, int k)
{
    const size_t l_pan = strlen(o->prior_an_tag), l_pac = strlen(o->prior_ac_tag);
    char *info = strdup(r->fld[7]); int ni; char **iv = split(info, ';', &ni);
    for (int i = 0; i < ni; ++i) {
        if (H->pan && !strncmp(iv[i], o->prior_an_tag, l_pan) && iv[i][l_pan] == '=') {        /* mcall.c:1499-1520 */
            if (!strchr(iv[i], ',')) H->pan[k] = atoi(iv[i] + l_pan + 1);
            continue;
        }
        if (H->pan && !strncmp(iv[i], o->prior_ac_tag, l_pac) && iv[i][l_pac] == '=') {
            char *c = strdup(iv[i] + l_pac + 1); int nv; char **v = split(c, ',', &nv);
            for (int j = 0; j < nv && j < 4; ++j) H->pac[(size_t)k * 4 + j] = !strcmp(v[j], ".") ? BCFGPU_INT32_MISSING : atoi(v[j]);
            free(v); free(c);
            continue;
        }
        const int is_qs = !strncmp(iv[i], "QS=", 3);
        if (!is_qs && strncmp(iv[i], "I16=", 4)) continue;
        float *dst = is_qs ? H->qs + (size_t)k * 5 : H->i16 + (size_t)k * 16;
        int nv; char **v = split(strchr(iv[i], '=') + 1, ',', &nv);
        for (int j = 0; j < nv && j < (is_qs ? 5 : 16); ++j) dst[j] = (float)atof(v[j]);
        free(v);
    }
    free(iv); free(info);
}
static void build_planes(const opt_t *o, const smap_t *M, recs_t *R, hplanes_t *H)
{
    const int n = R->n, S = M->S, ngmax = R->ngmax, namax = R->namax, dev_in = o->dev_in, on_dev = o->dev_in || o->dev_parse;
    memset(H, 0, sizeof *H);
    H->nals = malloc((size_t)n * 4); H->unseen = malloc((size_t)n * 4);
    H->pl = on_dev ? NULL : malloc((size_t)n * ngmax * S * 4);
    H->want_ad = M->ngrp > 1;
    H->vec_pl = dev_in ? calloc((size_t)n + 1, sizeof *H->vec_pl) : NULL; H->vec_ad = dev_in && H->want_ad ? calloc((size_t)n + 1, sizeof *H->vec_ad) : NULL;
    H->txt_pl = o->dev_parse ? calloc((size_t)n + 1, sizeof *H->txt_pl) : NULL; H->txt_ad = o->dev_parse && H->want_ad ? calloc((size_t)n + 1, sizeof *H->txt_ad) : NULL;
    H->qs = calloc((size_t)n * 5, 4); H->i16 = calloc((size_t)n * 16, 4);
    H->ad = H->want_ad && !on_dev ? malloc((size_t)n * namax * S * 4) : NULL;
    H->pan = o->prior_an_tag[0] ? malloc((size_t)n * 4) : NULL; H->pac = o->prior_an_tag[0] ? malloc((size_t)n * 4 * 4) : NULL;
    for (int k = 0; k < n; ++k) {
        rec_t *r = &R->rec[k];
        int32_t *pl = H->pl ? H->pl + (size_t)k * ngmax * S : NULL, *ad = H->ad ? H->ad + (size_t)k * namax * S : NULL;
        H->nals[k] = r->nals; H->unseen[k] = r->unseen;
        if (pl) for (size_t i = 0; i < (size_t)ngmax * S; ++i) pl[i] = BCFGPU_INT32_VECTOR_END;
        if (ad) for (size_t i = 0; i < (size_t)namax * S; ++i) ad[i] = BCFGPU_INT32_VECTOR_END;
        if (H->pan) { H->pan[k] = BCFGPU_INT32_MISSING; for (int i = 0; i < 4; ++i) H->pac[(size_t)k * 4 + i] = BCFGPU_INT32_VECTOR_END; }
        format_lookup(o, r, H->want_ad, dev_in ? &H->vec_pl[k] : NULL, H->vec_ad ? &H->vec_ad[k] : NULL, H->txt_pl ? &H->txt_pl[k] : NULL, H->txt_ad ? &H->txt_ad[k] : NULL);
        for (int s = 0; s < S && !on_dev; ++s) {
            char *smp = strdup(r->fld[9 + M->col[s]]); int nv; char **vals = split(smp, ':', &nv);
            parse_int_list(vals, nv, r->pl_idx, pl, ngmax, S, s);
            if (ad) parse_int_list(vals, nv, r->ad_idx, ad, namax, S, s);
            free(vals); free(smp);
        }
        parse_info(o, r, H, k);
    }
}

/* ---- the device ---- */
/* everything goes up once; the records are called in runs of equal ploidy vectors (the ploidy is per call:
 * vcfcall.c:807-825 re-initialises it when it changes) -- the planes are [record][...]: a run is a slice */
/* --device-parse: a record with the wrong number of columns, or a value that is no integer, is the text route's "malformed VCF" */
static void decode_text_planes(bcfgpu_ctx *ctx, int n, int S_in, const void *d_text, size_t l_text, const bcfgpu_vcf_vec *vec, const int32_t *cmap, int n_planes, int32_t *d_out)
{
    const int rc = bcfgpu_call_decode_vcf(ctx, n, S_in, d_text, l_text, vec, cmap, n_planes, d_out);
    if (rc == BCFGPU_E_ARG) DIE("malformed VCF\n");
    if (rc) DIE("bcfgpu_call_decode_vcf: %s (%d)\n", bcfgpu_last_error(), rc);
}
/* --device-alleles: the planes the decoders made in the input records' alleles (n_in a site, at d_in) become the planes mcall() reads,
 * in the targets' alleles (n_out a site); the input-shape planes are freed.  numberR: the -G tag's planes (a tag the header does not
 * declare Number=R stays as it is, as on the host) */
static int32_t *constrain_planes(bcfgpu_ctx *ctx, const recs_t *R, int S, int numberR, int follows, int n_in, int32_t *d_in, int n_out)
{
    void *dp = NULL;
    bcfgpu_cals_site *cs = calloc((size_t)R->n + 1, sizeof *cs);
    if (!cs) DIE("out of memory\n");
    for (int k = 0; k < R->n; ++k) {
        const rec_t *r = &R->rec[k];
        cs[k].n_new = r->nals; cs[k].unseen = r->unseen_in; cs[k].changed = r->changed && follows;
        for (int i = 0; i < BCFGPU_MAX_ALLELES; ++i) cs[k].amap[i] = r->amap[i];
    }
    CHECK(bcfgpu_malloc(ctx, (size_t)R->n * n_out * S * 4 + 16, &dp));
    const int rc = bcfgpu_call_constrain(ctx, numberR ? BCFGPU_CALS_NUMBER_R : BCFGPU_CALS_NUMBER_G, R->n, cs, n_in, d_in, n_out, dp);
    if (rc) DIE("bcfgpu_call_constrain: %s (%d)\n", bcfgpu_last_error(), rc);
    CHECK(bcfgpu_free(ctx, d_in));
    free(cs);
    return dp;
}
static void call_on_device(const opt_t *o, const ploidy_t *P, const smap_t *M, const recs_t *R, const hplanes_t *H, dev_t *D)
{
    const rec_t *recs = R->rec; const int n = R->n, S = M->S, ngmax = R->ngmax, namax = R->namax, dev_rec = o->dev_rec || o->dev_text;
    /* --device-alleles: the decoders write planes of the input records' shape, bcfgpu_call_constrain those of the constrained records */
    const int ngin = o->dev_als ? R->ngin : ngmax, nain = o->dev_als ? R->nain : namax;
    const int tag_is_R = o->grp_tag && is_numberR(fmtR, n_fmtR, o->grp_tag, strlen(o->grp_tag));
    memset(D, 0, sizeof *D);
    bcfgpu_cfg cfg; memset(&cfg, 0, sizeof cfg);
    cfg.device = 0; cfg.n_smpl = S; cfg.max_sites = n; cfg.max_reads = 64;
    cfg.min_baseQ = 13; cfg.capQ = 60; cfg.call_theta = o->prior; cfg.call_flag = (o->varonly ? BCFGPU_CALL_VARONLY : 0) | (o->keepalt ? BCFGPU_CALL_KEEPALT : 0); cfg.n_grp = M->ngrp;
    cfg.ploidy_max = P->max;                                     /* the prior's allele count is ploidy_max * S, whatever the samples' own ploidies */
    cfg.output_tags = o->out_tags;
    CHECK(bcfgpu_create(&cfg, &D->ctx)); bcfgpu_ctx *ctx = D->ctx;
    D->d_nals = dev_upload(ctx, H->nals, (size_t)n * 4); D->d_unseen = dev_upload(ctx, H->unseen, (size_t)n * 4);
    if (o->dev_in) {                                             /* the bytes go up once; the planes are made where mcall() reads them */
        void *dp = NULL;
        D->d_indiv = dev_upload(ctx, R->ibuf, R->ibuf_l);
        const int32_t *cmap = o->smpl_file ? (const int32_t *)M->col : NULL;     /* without -S / -s called sample s is input sample s */
        CHECK(bcfgpu_malloc(ctx, (size_t)n * ngin * S * 4 + 16, &dp)); D->d_plin = dp;
        CHECK(bcfgpu_call_decode_bcf(ctx, n, M->S_in, D->d_indiv, R->ibuf_l, H->vec_pl, cmap, ngin, D->d_plin));
        if (o->dev_als) D->d_plin = constrain_planes(ctx, R, S, 0, 1, ngin, D->d_plin, ngmax);
        if (H->want_ad) {
            CHECK(bcfgpu_malloc(ctx, (size_t)n * nain * S * 4 + 16, &dp)); D->d_ad = dp;
            CHECK(bcfgpu_call_decode_bcf(ctx, n, M->S_in, D->d_indiv, R->ibuf_l, H->vec_ad, cmap, nain, D->d_ad));
            if (o->dev_als) D->d_ad = constrain_planes(ctx, R, S, 1, tag_is_R, nain, D->d_ad, namax);
        }
        if (!o->dev_keys && !o->dev_text) { CHECK(bcfgpu_free(ctx, D->d_indiv)); D->d_indiv = NULL; }
    } else if (o->dev_parse) {                                   /* the columns' text goes up once and is parsed there */
        void *dp = NULL;
        D->d_indiv = dev_upload(ctx, R->ibuf, R->ibuf_l);
        const int32_t *cmap = o->smpl_file ? (const int32_t *)M->col : NULL;
        CHECK(bcfgpu_malloc(ctx, (size_t)n * ngin * S * 4 + 16, &dp)); D->d_plin = dp;
        decode_text_planes(ctx, n, M->S_in, D->d_indiv, R->ibuf_l, H->txt_pl, cmap, ngin, D->d_plin);
        if (o->dev_als) D->d_plin = constrain_planes(ctx, R, S, 0, 1, ngin, D->d_plin, ngmax);
        if (H->want_ad) {
            CHECK(bcfgpu_malloc(ctx, (size_t)n * nain * S * 4 + 16, &dp)); D->d_ad = dp;
            decode_text_planes(ctx, n, M->S_in, D->d_indiv, R->ibuf_l, H->txt_ad, cmap, nain, D->d_ad);
            if (o->dev_als) D->d_ad = constrain_planes(ctx, R, S, 1, tag_is_R, nain, D->d_ad, namax);
        }
        if (!o->dev_keys && !o->dev_text) { CHECK(bcfgpu_free(ctx, D->d_indiv)); D->d_indiv = NULL; }
    } else {
        D->d_plin = dev_upload(ctx, H->pl, (size_t)n * ngmax * S * 4);
        if (H->ad) D->d_ad = dev_upload(ctx, H->ad, (size_t)n * namax * S * 4);
    }
    D->d_qs = dev_upload(ctx, H->qs, (size_t)n * 5 * 4); D->d_i16 = dev_upload(ctx, H->i16, (size_t)n * 16 * 4);
    D->d_grp = M->grp ? dev_upload(ctx, M->grp, (size_t)S * 4) : NULL;
    D->d_pan = H->pan ? dev_upload(ctx, H->pan, (size_t)n * 4) : NULL; D->d_pac = H->pan ? dev_upload(ctx, H->pac, (size_t)n * 16) : NULL;
    if (o->out_tags & BCFGPU_CALL_FMT_GQ) CHECK(bcfgpu_malloc(ctx, (size_t)n * S * 4, &D->d_gq));
    if (o->out_tags & BCFGPU_CALL_FMT_GP) CHECK(bcfgpu_malloc(ctx, (size_t)n * ngmax * S * 4, &D->d_gp));
    CHECK(bcfgpu_malloc(ctx, (size_t)n * sizeof(bcfgpu_call_site), &D->d_site)); CHECK(bcfgpu_malloc(ctx, (size_t)n * 2 * S, &D->d_gt));
    CHECK(bcfgpu_malloc(ctx, (size_t)n * ngmax * S * 4, &D->d_pl)); CHECK(bcfgpu_malloc(ctx, (size_t)S + 16, &D->d_ploidy));
    for (int i = 0; i < n; ) {
        int j = i + 1, all2 = 1;
        while (j < n && !memcmp(recs[j].ploidy, recs[i].ploidy, (size_t)S)) ++j;
        for (int s = 0; s < S; ++s) all2 &= recs[i].ploidy[s] == 2;
        bcfgpu_call_in in; memset(&in, 0, sizeof in);
        in.n_sites = j - i; in.n_gt_max = ngmax; in.n_al_max = 0;
        in.nals = D->d_nals + i; in.unseen = D->d_unseen + i; in.pl = D->d_plin + (size_t)i * ngmax * S; in.qs = D->d_qs + (size_t)i * 5;
        in.i16 = D->d_i16 + (size_t)i * 16;
        if (D->d_ad) { in.ad = D->d_ad + (size_t)i * namax * S; in.n_al_max = namax; in.grp = D->d_grp; }
        if (D->d_pan) { in.prior_an = D->d_pan + i; in.prior_ac = D->d_pac + (size_t)i * 4; }
        if (!all2) { CHECK(bcfgpu_memcpy_h2d(ctx, D->d_ploidy, recs[i].ploidy, (size_t)S)); in.ploidy = D->d_ploidy; }
        bcfgpu_call_out out; memset(&out, 0, sizeof out);
        out.site = (bcfgpu_call_site*)D->d_site + i; out.gt = (int8_t*)D->d_gt + (size_t)i * 2 * S; out.pl = (int32_t*)D->d_pl + (size_t)i * ngmax * S;
        if (D->d_gq) out.gq = (int32_t*)D->d_gq + (size_t)i * S;
        if (D->d_gp) out.gp = (float*)D->d_gp + (size_t)i * ngmax * S;
        CHECK(bcfgpu_mcall(ctx, &in, &out));
        CHECK(bcfgpu_sync(ctx));                                      /* (d_ploidy is reused by the next run) */
        i = j;
    }
    D->cs = malloc((size_t)n * sizeof *D->cs);
    /* --device-records: the site records alone come down here (and GP); GT, PL and GQ follow as bytes once the writer's header is known.
     * --device-text (on either kind of input): the site records alone; the planes follow only when a written record is left to the host
     * (download_planes) */
    D->gt = dev_rec ? NULL : malloc((size_t)n * 2 * S); D->opl = dev_rec ? NULL : malloc((size_t)n * ngmax * S * 4);
    CHECK(bcfgpu_memcpy_d2h(ctx, D->cs, D->d_site, (size_t)n * sizeof *D->cs));
    if (D->gt) CHECK(bcfgpu_memcpy_d2h(ctx, D->gt, D->d_gt, (size_t)n * 2 * S));
    if (D->opl) CHECK(bcfgpu_memcpy_d2h(ctx, D->opl, D->d_pl, (size_t)n * ngmax * S * 4));
    D->gq = D->d_gq && !dev_rec ? malloc((size_t)n * S * 4) : NULL; D->gp = D->d_gp && !o->dev_text ? malloc((size_t)n * ngmax * S * 4) : NULL;
    if (D->gq) CHECK(bcfgpu_memcpy_d2h(ctx, D->gq, D->d_gq, (size_t)n * S * 4));
    if (D->gp) CHECK(bcfgpu_memcpy_d2h(ctx, D->gp, D->d_gp, (size_t)n * ngmax * S * 4));
    CHECK(bcfgpu_sync(ctx));
}

/* ---- the output header: the input's, for the samples kept, without the calling-only tags, plus what mcall_init
 * declares (vcfcall.c:670,703-704; mcall.c:382-394) ---- */
static void output_header(const opt_t *o, const smap_t *M, vio_hdr *hdr)
{
    if (o->smpl_file && vio_hdr_subset(hdr, M->S, M->col)) DIE("%s\n", vio_error());
    vio_hdr_remove(hdr, "INFO", "QS");
    vio_hdr_remove(hdr, "INFO", "I16");
    if (o->gv_n) {                                               /* gvcf_update_header, on the reader's header (vcfcall.c:661-666) */
        vio_hdr_append(hdr, "##INFO=<ID=END,Number=1,Type=Integer,Description=\"End position of the variant described in this record\">");
        vio_hdr_append(hdr, "##INFO=<ID=MinDP,Number=1,Type=Integer,Description=\"Minimum per-sample depth in this gVCF block\">");
    }
    vio_hdr_append(hdr, "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">");
    if (o->out_tags & BCFGPU_CALL_FMT_GQ) vio_hdr_append(hdr, "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Phred-scaled Genotype Quality\">");
    if (o->out_tags & BCFGPU_CALL_FMT_GP) vio_hdr_append(hdr, "##FORMAT=<ID=GP,Number=G,Type=Float,Description=\"Genotype posterior probabilities in the range 0 to 1\">");
    vio_hdr_append(hdr, "##INFO=<ID=AC,Number=A,Type=Integer,Description=\"Allele count in genotypes for each ALT allele, in the same order as listed\">");
    vio_hdr_append(hdr, "##INFO=<ID=AN,Number=1,Type=Integer,Description=\"Total number of alleles in called genotypes\">");
    vio_hdr_append(hdr, "##INFO=<ID=DP4,Number=4,Type=Integer,Description=\"Number of high-quality ref-forward , ref-reverse, alt-forward and alt-reverse bases\">");
    vio_hdr_append(hdr, "##INFO=<ID=MQ,Number=1,Type=Integer,Description=\"Average mapping quality\">");
}

/* ---- --device-records: GT, PL and GQ of the records that will be written, as BCF2 key blocks made in HBM; the key ids are the
 * output header's.  One call over all records: the size first, then the bytes; one offset per record and key ---- */
typedef struct { bcfgpu_ctx *ctx; int n, ngmax; bcfgpu_call_out planes; int32_t kid[BCFGPU_CALL_BCF_NKEYS]; const void *d_emit; } enc_arg;
static int enc_call(void *arg, void *d_buf, uint64_t cap, uint64_t *d_off, uint64_t *need)
{
    const enc_arg *a = arg;
    return bcfgpu_call_encode_bcf(a->ctx, a->n, a->ngmax, &a->planes, a->kid, a->d_emit, d_buf, cap, d_off, need);
}
static void encode_call_blocks(const opt_t *o, const recs_t *R, const dev_t *D, const vio_hdr *hdr, blocks_t *B)
{
    const int n = R->n;
    B->emit = malloc((size_t)n + 1);
    for (int k = 0; k < n; ++k) { B->emit[k] = !(D->cs[k].ret < 0 || (o->varonly && D->cs[k].ret == 0)); B->n_enc += B->emit[k]; }      /* the record loop's rule */
    enc_arg a; memset(&a, 0, sizeof a);
    a.ctx = D->ctx; a.n = n; a.ngmax = R->ngmax;
    a.kid[BCFGPU_CALL_BCF_GT] = vio_hdr_fmt_id(hdr, "GT"); a.kid[BCFGPU_CALL_BCF_PL] = vio_hdr_fmt_id(hdr, "PL");
    a.kid[BCFGPU_CALL_BCF_GQ] = D->d_gq ? vio_hdr_fmt_id(hdr, "GQ") : 0;
    if (a.kid[BCFGPU_CALL_BCF_PL] < 0) DIE("FORMAT tag PL is not defined in the header\n");
    a.d_emit = B->d_emit = dev_upload(D->ctx, B->emit, (size_t)n);
    a.planes.site = D->d_site; a.planes.gt = D->d_gt; a.planes.pl = D->d_pl; a.planes.gq = D->d_gq;
    encode_two_pass(D->ctx, enc_call, &a, "bcfgpu_call_encode_bcf", (size_t)n * BCFGPU_CALL_BCF_NKEYS + 1, &B->kblk, &B->koff);
}

/* ---- --device-keys: a job for every integer pass-through key of every record that is written; the blocks are made from the
 * input's bytes where --device-input left them, with the sample map it passed and the site records' als_map ---- */
typedef struct { bcfgpu_ctx *ctx; int32_t n_job; const bcfgpu_bcf_key *job; int S_in, n; const void *d_indiv; size_t l_indiv; const int32_t *cmap; const void *d_site, *d_emit; } remap_arg;
static int remap_call(void *arg, void *d_buf, uint64_t cap, uint64_t *d_off, uint64_t *need)
{
    const remap_arg *a = arg;
    return bcfgpu_call_remap_bcf(a->ctx, a->n_job, a->job, a->S_in, a->d_indiv, a->l_indiv, a->cmap, a->d_site, a->n, a->d_emit, d_buf, cap, d_off, need);
}
/* the same on text input (--device-parse): the jobs come from the record's FORMAT column, the blocks from the columns' text where
 * --device-parse left it.  A job the device flags (a value outside the exact integer grammar, a key wider than 255 values) goes back to
 * the host: its block has zero length and the text route makes the key */
typedef struct { bcfgpu_ctx *ctx; int32_t n_job; const bcfgpu_vcf_key *job; int n; const bcfgpu_vcf_vec *run; int S_in; const void *d_text; size_t l_text; const int32_t *cmap;
                 const void *d_site, *d_emit; uint8_t *status; } parse_keys_arg;
static int parse_keys_call(void *arg, void *d_buf, uint64_t cap, uint64_t *d_off, uint64_t *need)
{
    const parse_keys_arg *a = arg;
    return bcfgpu_call_parse_keys_vcf(a->ctx, a->n_job, a->job, a->n, a->run, a->S_in, a->d_text, a->l_text, a->cmap, a->d_site, a->d_emit, d_buf, cap, d_off, need, a->status);
}
static void parse_key_blocks(const opt_t *o, const smap_t *M, recs_t *R, const hplanes_t *H, dev_t *D, const vio_hdr *hdr, blocks_t *B)
{
    size_t cap_job = 0; bcfgpu_vcf_key *job = NULL;
    for (int k = 0; k < R->n; ++k) {
        rec_t *r = &R->rec[k];
        if (!B->emit[k]) continue;
        int nk; char *fmt = strdup(r->fld[8]), **keys = split(fmt, ':', &nk);
        r->kjob = malloc((size_t)nk * sizeof *r->kjob); r->nkjob = nk;
        for (int i = 0; i < nk; ++i) {
            r->kjob[i] = -1;
            if (i == r->pl_idx || i >= BCFGPU_VCF_REWRITE_MAX_KEYS || !strcmp(keys[i], "GT")) continue;
            const int id = vio_hdr_fmt_id(hdr, keys[i]);
            if (id < 0 || vio_hdr_fmt_type(hdr, id) != VIO_TYPE_INT) continue;
            if (r->changed && is_numberR(fmtR, n_fmtR, keys[i], strlen(keys[i]))) continue;      /* --device-alleles: the key follows amap first: the host's */
            if ((size_t)B->n_pjob == cap_job) { cap_job = cap_job ? 2 * cap_job : 4096; job = realloc(job, cap_job * sizeof *job); if (!job) DIE("out of memory\n"); }
            bcfgpu_vcf_key *j = &job[B->n_pjob];
            memset(j, 0, sizeof *j);
            j->site = k; j->key_id = id; j->idx = i; j->nals = r->nals;
            j->flags = is_numberR(fmtR, n_fmtR, keys[i], strlen(keys[i]));
            r->kjob[i] = (int)B->n_pjob++;
        }
        free(keys); free(fmt);
    }
    if (B->n_pjob > INT32_MAX - 1) DIE("too many pass-through keys for one call\n");
    if (B->n_pjob) {
        uint8_t *status = calloc((size_t)B->n_pjob, 1);
        parse_keys_arg a = { D->ctx, (int32_t)B->n_pjob, job, R->n, H->txt_pl, M->S_in, D->d_indiv, R->ibuf_l, o->smpl_file ? (const int32_t *)M->col : NULL, D->d_site, B->d_emit, status };
        encode_two_pass(D->ctx, parse_keys_call, &a, "bcfgpu_call_parse_keys_vcf", (size_t)B->n_pjob + 1, &B->pblk, &B->poff);
        long n_flagged = 0;
        for (long j = 0; j < B->n_pjob; ++j) n_flagged += status[j] != 0;
        for (int k = 0; n_flagged && k < R->n; ++k) {              /* the flagged jobs are the host's again */
            rec_t *r = &R->rec[k];
            for (int i = 0; r->kjob && i < r->nkjob; ++i) if (r->kjob[i] >= 0 && status[r->kjob[i]]) r->kjob[i] = -1;
        }
        B->n_pjob -= n_flagged;                                  /* (write_record counts them under the host's) */
        free(status);
    } else B->poff = calloc(1, 8);
    free(job);
    CHECK(bcfgpu_free(D->ctx, D->d_indiv)); D->d_indiv = NULL;
}
static void encode_key_blocks(const opt_t *o, const smap_t *M, recs_t *R, const hplanes_t *H, dev_t *D, const vio_hdr *hdr, blocks_t *B)
{
    if (o->dev_parse) { parse_key_blocks(o, M, R, H, D, hdr, B); return; }
    size_t cap_job = 0; bcfgpu_bcf_key *job = NULL;
    for (int k = 0; k < R->n; ++k) {
        rec_t *r = &R->rec[k];
        if (!B->emit[k]) continue;
        r->kjob = malloc((size_t)(r->nkeys ? r->nkeys : 1) * sizeof *r->kjob); r->nkjob = r->nkeys;
        for (int i = 0; i < r->nkeys; ++i) {
            const vio_indiv_key *q = &r->keys[i];
            r->kjob[i] = -1;
            if (i == r->pl_idx || !strcmp(q->id, "GT") || vio_hdr_fmt_type(hdr, q->dict) != VIO_TYPE_INT) continue;
            if (q->type < 0 || q->type > 3 || q->width < 0 || q->width > BCFGPU_BCF_KEY_MAX_WIDTH) continue;
            const int id = vio_hdr_fmt_id(hdr, q->id);
            if (id < 0) continue;
            if (r->changed && is_numberR(fmtR, n_fmtR, q->id, strlen(q->id))) continue;          /* --device-alleles: the key follows amap first: the host's */
            if ((size_t)B->n_pjob == cap_job) { cap_job = cap_job ? 2 * cap_job : 4096; job = realloc(job, cap_job * sizeof *job); if (!job) DIE("out of memory\n"); }
            bcfgpu_bcf_key *j = &job[B->n_pjob];
            j->off = r->ioff + q->off; j->site = k; j->key_id = id; j->type = q->type; j->width = q->width; j->nals = r->nals;
            j->flags = is_numberR(fmtR, n_fmtR, q->id, strlen(q->id));
            r->kjob[i] = (int)B->n_pjob++;
        }
    }
    if (B->n_pjob > INT32_MAX - 1) DIE("too many pass-through keys for one call\n");
    if (B->n_pjob) {
        remap_arg a = { D->ctx, (int32_t)B->n_pjob, job, M->S_in, R->n, D->d_indiv, R->ibuf_l, o->smpl_file ? (const int32_t *)M->col : NULL, D->d_site, B->d_emit };
        encode_two_pass(D->ctx, remap_call, &a, "bcfgpu_call_remap_bcf", (size_t)B->n_pjob + 1, &B->pblk, &B->poff);
    } else B->poff = calloc(1, 8);
    free(job);
    CHECK(bcfgpu_free(D->ctx, D->d_indiv)); D->d_indiv = NULL;
}

/* ---- --device-text: the sample columns of the records that are written, as VCF text made in HBM from the call planes and the
 * input's bytes where --device-input left them.  A field list per record in the order of its FORMAT column; a record the device
 * cannot format (see the head of this file) has no field and d_emit = 0: the host's route writes it, from planes that come down only
 * then ---- */
typedef struct { bcfgpu_ctx *ctx; int n, ngmax; bcfgpu_call_out planes; int32_t n_field; const bcfgpu_vcf_field *field; int S_in; const void *d_indiv; size_t l_indiv;
                 const int32_t *cmap; const void *d_emit; } text_arg;
static int text_call(void *arg, void *d_buf, uint64_t cap, uint64_t *d_off, uint64_t *need)
{
    const text_arg *a = arg;
    return bcfgpu_call_encode_vcf(a->ctx, a->n, a->ngmax, &a->planes, a->n_field, a->field, a->S_in, a->d_indiv, a->l_indiv, a->cmap, a->d_emit, d_buf, cap, d_off, need);
}
/* values x (longest text of a value + 1): a pass-through key's share of the bound on one sample's text (include/bcfgpu.h) */
static size_t key_text_bound(const bcfgpu_vcf_field *f)
{
    size_t values = f->type && f->width > 1 ? (size_t)f->width : 1;
    if ((f->flags & 1) && values < BCFGPU_MAX_ALLELES) values = BCFGPU_MAX_ALLELES;
    return values * (f->type == 3 ? 12u : f->type == 2 ? 7u : 5u);
}
static void download_planes(const smap_t *M, const recs_t *R, dev_t *D)
{
    const size_t n = (size_t)R->n, S = (size_t)M->S, ngmax = (size_t)R->ngmax;
    D->gt = malloc(n * 2 * S + 1); D->opl = malloc(n * ngmax * S * 4 + 1);
    CHECK(bcfgpu_memcpy_d2h(D->ctx, D->gt, D->d_gt, n * 2 * S)); CHECK(bcfgpu_memcpy_d2h(D->ctx, D->opl, D->d_pl, n * ngmax * S * 4));
    if (D->d_gq) { D->gq = malloc(n * S * 4 + 1); CHECK(bcfgpu_memcpy_d2h(D->ctx, D->gq, D->d_gq, n * S * 4)); }
    if (D->d_gp) { D->gp = malloc(n * ngmax * S * 4 + 1); CHECK(bcfgpu_memcpy_d2h(D->ctx, D->gp, D->d_gp, n * ngmax * S * 4)); }
    CHECK(bcfgpu_sync(D->ctx));
}
static void encode_text_columns(const opt_t *o, const smap_t *M, const recs_t *R, dev_t *D, blocks_t *B)
{
    const int n = R->n;
    uint8_t *emit = malloc((size_t)n + 1);
    size_t cap_f = 0, n_f = 0; bcfgpu_vcf_field *fld = NULL; long n_host = 0;
    for (int k = 0; k < n; ++k) {
        const rec_t *r = &R->rec[k]; const bcfgpu_call_site *c = &D->cs[k];
        emit[k] = 0;
        if (c->ret < 0 || (o->varonly && c->ret == 0)) continue;                /* the record loop's rule: not written */
        const int called = c->nals_new > 1 && c->ret > 0;
        const int n_here = 1 + r->nkeys - (c->pl_dropped ? 1 : 0) + (called && D->d_gq ? 1 : 0);
        int ok = r->nkeys == r->n_fmt && !(called && D->d_gp) && n_here <= BCFGPU_VCF_MAX_FIELDS;
        for (int i = 0; ok && i < r->nkeys; ++i) {
            const vio_indiv_key *q = &r->keys[i];
            if (!strcmp(q->id, "GT")) ok = 0;
            else if (i != r->pl_idx && (q->type < 0 || q->type > 3 || q->width < 0 || q->width > BCFGPU_BCF_KEY_MAX_WIDTH)) ok = 0;
            else if (i != r->pl_idx && r->changed && is_numberR(fmtR, n_fmtR, q->id, strlen(q->id))) ok = 0;      /* --device-alleles: a key that follows amap first */
        }
        if (ok) {
            if (n_f + BCFGPU_VCF_MAX_FIELDS > cap_f) { cap_f = cap_f ? 2 * cap_f : 4096; fld = realloc(fld, cap_f * sizeof *fld); if (!fld) DIE("out of memory\n"); }
            const size_t f0 = n_f; size_t bound = 1 + 4;
            bcfgpu_vcf_field *f = &fld[n_f++];
            memset(f, 0, sizeof *f); f->site = k; f->kind = BCFGPU_VCF_FIELD_GT;
            for (int i = 0; i < r->nkeys; ++i) {
                const vio_indiv_key *q = &r->keys[i];
                if (i == r->pl_idx && c->pl_dropped) continue;
                f = &fld[n_f++];
                memset(f, 0, sizeof *f); f->site = k;
                if (i == r->pl_idx) { f->kind = BCFGPU_VCF_FIELD_PL; bound += (size_t)R->ngmax * 12; continue; }
                f->kind = BCFGPU_VCF_FIELD_KEY; f->off = r->ioff + q->off; f->type = q->type; f->width = q->width; f->nals = r->nals;
                f->flags = is_numberR(fmtR, n_fmtR, q->id, strlen(q->id));
                bound += key_text_bound(f);
            }
            if (called && D->d_gq) { f = &fld[n_f++]; memset(f, 0, sizeof *f); f->site = k; f->kind = BCFGPU_VCF_FIELD_GQ; bound += 12; }
            if (bound > BCFGPU_VCF_SAMPLE_CAP) { ok = 0; n_f = f0; }
        }
        emit[k] = (uint8_t)ok;
        if (ok) ++B->n_tdev; else ++n_host;
    }
    if (n_f > INT32_MAX - 1) DIE("too many fields for one call\n");
    text_arg a; memset(&a, 0, sizeof a);
    a.ctx = D->ctx; a.n = n; a.ngmax = R->ngmax; a.n_field = (int32_t)n_f; a.field = fld; a.S_in = M->S_in; a.d_indiv = D->d_indiv; a.l_indiv = R->ibuf_l;
    a.cmap = o->smpl_file ? (const int32_t *)M->col : NULL;
    void *d_emit = dev_upload(D->ctx, emit, (size_t)n); a.d_emit = d_emit;
    a.planes.site = D->d_site; a.planes.gt = D->d_gt; a.planes.pl = D->d_pl; a.planes.gq = D->d_gq;
    encode_two_pass(D->ctx, text_call, &a, "bcfgpu_call_encode_vcf", (size_t)n + 1, &B->tblk, &B->toff);
    CHECK(bcfgpu_free(D->ctx, d_emit)); CHECK(bcfgpu_free(D->ctx, D->d_indiv)); D->d_indiv = NULL;
    free(fld); free(emit);
    if (n_host) download_planes(M, R, D);                       /* (GP with them: a record that carries it is the host's) */
}

/* ---- --device-text on text input: the same columns rewritten in HBM from the input's own text where --device-parse left it.  One
 * bcfgpu_vcf_rewrite per record; a record the device does not rewrite (GP, a key named GT, more than 64 keys) has d_emit = 0 and a
 * record that only describes its run: the host's route writes it, from planes that come down only then ---- */
typedef struct { bcfgpu_ctx *ctx; int n, ngmax; bcfgpu_call_out planes; const bcfgpu_vcf_rewrite *rec; int S_in; const void *d_text; size_t l_text;
                 const int32_t *cmap; const void *d_emit; } rewrite_arg;
static int rewrite_call(void *arg, void *d_buf, uint64_t cap, uint64_t *d_off, uint64_t *need)
{
    const rewrite_arg *a = arg;
    return bcfgpu_call_rewrite_vcf(a->ctx, a->n, a->ngmax, &a->planes, a->rec, a->S_in, a->d_text, a->l_text, a->cmap, a->d_emit, d_buf, cap, d_off, need);
}
static void rewrite_text_columns(const opt_t *o, const smap_t *M, const recs_t *R, dev_t *D, blocks_t *B)
{
    const int n = R->n;
    uint8_t *emit = malloc((size_t)n + 1);
    bcfgpu_vcf_rewrite *rw = calloc((size_t)n + 1, sizeof *rw); long n_host = 0;
    if (!rw) DIE("out of memory\n");
    for (int k = 0; k < n; ++k) {
        const rec_t *r = &R->rec[k]; const bcfgpu_call_site *c = &D->cs[k];
        bcfgpu_vcf_rewrite *w = &rw[k];
        w->off = r->ioff; w->len = (uint32_t)r->ilen; w->pl_idx = -1; w->n_fmt = 1; w->nals = (int16_t)r->nals;
        emit[k] = 0;
        if (c->ret < 0 || (o->varonly && c->ret == 0)) continue;                /* the record loop's rule: not written */
        const int called = c->nals_new > 1 && c->ret > 0;
        int nk; char *fmt = strdup(r->fld[8]), **keys = split(fmt, ':', &nk);
        int ok = !(called && D->d_gp) && nk <= BCFGPU_VCF_REWRITE_MAX_KEYS;
        for (int i = 0; ok && i < nk; ++i) if (!strcmp(keys[i], "GT")) ok = 0;
        for (int i = 0; ok && r->changed && i < nk; ++i) if (i != r->pl_idx && is_numberR(fmtR, n_fmtR, keys[i], strlen(keys[i]))) ok = 0;   /* --device-alleles: a key that follows amap first */
        if (ok) {
            w->n_fmt = (int16_t)nk; w->pl_idx = r->pl_idx;
            for (int i = 0; i < nk; ++i) if (is_numberR(fmtR, n_fmtR, keys[i], strlen(keys[i]))) w->r_mask |= 1ull << i;
            w->flags = (c->pl_dropped ? 0 : 1) | (called && D->d_gq ? 2 : 0);
        }
        free(keys); free(fmt);
        emit[k] = (uint8_t)ok;
        if (ok) ++B->n_tdev; else ++n_host;
    }
    rewrite_arg a; memset(&a, 0, sizeof a);
    a.ctx = D->ctx; a.n = n; a.ngmax = R->ngmax; a.rec = rw; a.S_in = M->S_in; a.d_text = D->d_indiv; a.l_text = R->ibuf_l;
    a.cmap = o->smpl_file ? (const int32_t *)M->col : NULL;
    void *d_emit = dev_upload(D->ctx, emit, (size_t)n); a.d_emit = d_emit;
    a.planes.site = D->d_site; a.planes.gt = D->d_gt; a.planes.pl = D->d_pl; a.planes.gq = D->d_gq;
    encode_two_pass(D->ctx, rewrite_call, &a, "bcfgpu_call_rewrite_vcf", (size_t)n + 1, &B->tblk, &B->toff);
    CHECK(bcfgpu_free(D->ctx, d_emit)); CHECK(bcfgpu_free(D->ctx, D->d_indiv)); D->d_indiv = NULL;
    free(rw); free(emit);
    if (n_host) download_planes(M, R, D);                       /* (GP with them: a record that carries it is the host's) */
}

/* ---- -g: gVCF blocks over the records that are written (vcfcall.c:1145-1149; gvcf_write, gvcf.c:88-226).  What
 * gvcf_write looks at goes to the device as arrays: may the record join (mcall() returned 1: the reference allele alone),
 * FORMAT/DP of every sample, position, sequence, INFO/END; the block table and the blocks' DP come back. ---- */
static void gvcf_blocks(const opt_t *o, const smap_t *M, const recs_t *R, const dev_t *D, gvcf_t *G)
{
    bcfgpu_ctx *ctx = D->ctx; const int n = R->n, S = M->S;
    int gv_nw = 0;
    G->w = malloc((size_t)(n + 1) * 4);
    int32_t *pos = malloc((size_t)(n + 1) * 4), *rid = malloc((size_t)(n + 1) * 4), *endp = malloc((size_t)(n + 1) * 4);
    uint8_t *ro = malloc((size_t)n + 1); int32_t *dp = malloc(((size_t)n * S + 1) * 4);
    char **chroms = NULL; int nchrom = 0;
    for (int k = 0; k < n; ++k) {
        const rec_t *r = &R->rec[k];
        if (D->cs[k].ret < 0) { G->w[k] = -1; continue; }
        const int w = G->w[k] = gv_nw++;
        pos[w] = atoi(r->fld[1]) - 1; endp[w] = pos[w];
        int ci; for (ci = 0; ci < nchrom; ++ci) if (!strcmp(chroms[ci], r->fld[0])) break;
        if (ci == nchrom) { chroms = realloc(chroms, (size_t)(nchrom + 1) * sizeof *chroms); chroms[nchrom++] = r->fld[0]; }
        rid[w] = ci;
        ro[w] = D->cs[k].ret == 1;
        const char *e = strstr(r->fld[7], "END=");
        if (e && (e == r->fld[7] || e[-1] == ';')) endp[w] = atoi(e + 4) - 1;
        int nk, dpi = -1; char *fmt = strdup(r->fld[8]), **keys = split(fmt, ':', &nk);
        for (int i = 0; i < nk; ++i) if (!strcmp(keys[i], "DP")) dpi = i;
        free(keys); free(fmt);
        for (int s2 = 0; s2 < S; ++s2) {
            int32_t v = INT32_MIN;                           /* missing: the record stays as it is */
            if (dpi >= 0) {
                char *smp = strdup(r->fld[9 + M->col[s2]]); int nv; char **vals = split(smp, ':', &nv);
                if (dpi < nv && strcmp(vals[dpi], ".")) v = atoi(vals[dpi]);
                free(vals); free(smp);
            }
            dp[(size_t)w * S + s2] = v;
        }
    }
    free(chroms);
    if (gv_nw) {
        void *d_pos = dev_upload(ctx, pos, (size_t)gv_nw * 4), *d_rid = dev_upload(ctx, rid, (size_t)gv_nw * 4), *d_end = dev_upload(ctx, endp, (size_t)gv_nw * 4);
        void *d_ro = dev_upload(ctx, ro, (size_t)gv_nw), *d_dp = dev_upload(ctx, dp, (size_t)gv_nw * S * 4);
        void *d_blk, *d_min, *d_block, *d_gdp;
        CHECK(bcfgpu_malloc(ctx, (size_t)gv_nw * 4, &d_blk)); CHECK(bcfgpu_malloc(ctx, (size_t)gv_nw * 4, &d_min));
        CHECK(bcfgpu_malloc(ctx, (size_t)gv_nw * sizeof(bcfgpu_gvcf_block), &d_block)); CHECK(bcfgpu_malloc(ctx, (size_t)gv_nw * S * 4, &d_gdp));
        bcfgpu_gvcf_in gi; memset(&gi, 0, sizeof gi);
        gi.n_sites = gv_nw; gi.n_range = o->gv_n; gi.dp_range = o->gv_range; gi.pos = d_pos; gi.rid = d_rid; gi.end = d_end; gi.ref_only = d_ro; gi.dp = d_dp;
        bcfgpu_gvcf_out go; memset(&go, 0, sizeof go);
        go.blk = d_blk; go.min_dp = d_min; go.block = d_block; go.dp = d_gdp;
        int32_t nb = 0;
        CHECK(bcfgpu_gvcf_blocks(ctx, &gi, &go, &nb));
        G->blk = malloc((size_t)gv_nw * 4); G->min = malloc((size_t)gv_nw * 4);
        G->block = malloc((size_t)(nb + 1) * sizeof *G->block); G->dp = malloc(((size_t)nb * S + 1) * 4);
        CHECK(bcfgpu_memcpy_d2h(ctx, G->blk, d_blk, (size_t)gv_nw * 4)); CHECK(bcfgpu_memcpy_d2h(ctx, G->min, d_min, (size_t)gv_nw * 4));
        if (nb) { CHECK(bcfgpu_memcpy_d2h(ctx, G->block, d_block, (size_t)nb * sizeof *G->block)); CHECK(bcfgpu_memcpy_d2h(ctx, G->dp, d_gdp, (size_t)nb * S * 4)); }
        CHECK(bcfgpu_sync(ctx));
    }
    free(pos); free(rid); free(endp); free(ro); free(dp);
}

/* ---- the record loop (vcfcall.c:1137-1147, mcall.c:1627-1681) ---- */
typedef struct {
    const opt_t *o; const smap_t *M; const recs_t *R; const dev_t *D; blocks_t *B; const gvcf_t *G; vio_file *fout; vio_hdr *hdr;
    char *smp_text; size_t smp_cap;
    char *hblk, *iblk; size_t hblk_cap, iblk_cap;                /* --device-records: the host keys' blocks, the record's per-sample part */
} writer_t;
/* what a record's FORMAT column says of its keys: who makes which */
typedef struct { char **keys; int nk, called, host_keys; const int *kjob; } fmt_t;
/* -i: a target that met no record (tgt_flush_region, vcfcall.c:408-424) */
static void write_missed_target(const writer_t *W, const tgt_t *t)
{
    fprintf(LN, "%s\t%d\t.\t%s\t", t->chrom, t->pos, t->als[0]);
    if (t->nals < 2) fputc('.', LN);
    for (int i = 1; i < t->nals; ++i) fprintf(LN, "%s%s", i > 1 ? "," : "", t->als[i]);
    fputs("\t.\t.\t.\tGT", LN);
    for (int s2 = 0; s2 < W->M->S; ++s2) fputs("\t.", LN);
    end_record(W->fout, W->hdr);
}
/* ALT: the kept alleles in their new order */
static void print_alt(const rec_t *r, const bcfgpu_call_site *c)
{
    const char *al[5] = { 0, 0, 0, 0, 0 };
    for (int i = 0; i < r->nals; ++i) if (c->als_map[i] >= 0) al[c->als_map[i]] = r->als[i];
    if (c->nals_new < 2) fputc('.', LN);
    for (int i = 1; i < c->nals_new; ++i) fprintf(LN, "%s%s", i > 1 ? "," : "", al[i]);
}
static void print_gt(const int8_t *gt, size_t k, int S, int s)
{
    const int g0 = gt[(k * 2 + 0) * S + s], g1 = gt[(k * 2 + 1) * S + s];
    if (g0 == BCFGPU_GT_MISSING) fputc('.', LN); else fprintf(LN, "%d", g0);
    if (g1 != BCFGPU_GT_VECTOR_END) { fputc('/', LN); if (g1 == BCFGPU_GT_MISSING) fputc('.', LN); else fprintf(LN, "%d", g1); }
}
/* record k closes block b: the block's one line (gvcf.c:134-166) */
static void write_block_line(const writer_t *W, int k, int b)
{
    const bcfgpu_gvcf_block *B = &W->G->block[b]; const int S = W->M->S;
    int kf = k; while (W->G->w[kf] != B->first_site) --kf;      /* the block's first record: alleles and genotypes are its */
    const rec_t *rf = &W->R->rec[kf];
    fprintf(LN, "%s\t%d\t.\t%s\t", rf->fld[0], B->start_pos + 1, rf->fld[3]);
    print_alt(rf, &W->D->cs[kf]);
    fputs("\t.\t.\t", LN);
    if (B->start_pos + 1 < B->end1) fprintf(LN, "END=%d;", B->end1);
    fprintf(LN, "MinDP=%d\tGT:DP", B->min_dp);
    for (int s2 = 0; s2 < S; ++s2) {
        fputc('\t', LN);
        print_gt(W->D->gt, (size_t)kf, S, s2);
        const int32_t v = W->G->dp[(size_t)b * S + s2];
        if (v == INT32_MIN) fputs(":.", LN); else fprintf(LN, ":%d", v);
    }
    end_record(W->fout, W->hdr);
}
/* INFO: I16 and QS go, AC / AN / DP4 / MQ come */
static void print_info(const rec_t *r, const bcfgpu_call_site *c, int gv_min_dp)
{
    const int nn = c->nals_new;
    char *info = strdup(r->fld[7]); int ni, first = 1; char **iv = split(info, ';', &ni);
    for (int i = 0; i < ni; ++i) {
        if (!strncmp(iv[i], "I16=", 4) || !strncmp(iv[i], "QS=", 3) || !strcmp(iv[i], ".")) continue;
        const char *eq = strchr(iv[i], '=');
        if (eq && nn != r->nals && is_numberR(infoR, n_infoR, iv[i], (size_t)(eq - iv[i]))) {
            fprintf(LN, "%s%.*s=", first ? "" : ";", (int)(eq - iv[i]), iv[i]);
            print_numberR(eq + 1, c->als_map, r->nals, nn);
        } else fprintf(LN, "%s%s", first ? "" : ";", iv[i]);
        first = 0;
    }
    free(iv); free(info);
    if (nn > 1) { fprintf(LN, "%sAC=", first ? "" : ";"); first = 0; for (int i = 1; i < nn; ++i) fprintf(LN, "%s%d", i > 1 ? "," : "", c->ac[i]); }
    fprintf(LN, "%sAN=%d", first ? "" : ";", c->an);
    if (c->has_i16) {
        fprintf(LN, ";DP4=%d,%d,%d,%d", c->dp4[0], c->dp4[1], c->dp4[2], c->dp4[3]);
        if (c->mq == BCFGPU_INT32_MISSING) fputs(";MQ=.", LN); else fprintf(LN, ";MQ=%d", c->mq);
    }
    if (gv_min_dp == INT32_MIN) fputs(";MinDP=.", LN); else if (gv_min_dp) fprintf(LN, ";MinDP=%d", gv_min_dp);
}
/* sample s of record k: GT (unless it is a block already), the input's keys the host makes, GP, GQ */
static void print_sample_text(const writer_t *W, int k, const fmt_t *F, const char *column, int s)
{
    const rec_t *r = &W->R->rec[k]; const bcfgpu_call_site *c = &W->D->cs[k]; const dev_t *D = W->D;
    const int S = W->M->S, ngmax = W->R->ngmax, dev_rec = W->o->dev_rec, nn = c->nals_new, ngn = nn * (nn + 1) / 2;
    int nf = 0;                                          /* fields of this sample so far: ':' in front of all but the first */
    if (!dev_rec || s) fputc('\t', LN);
    if (!dev_rec) { print_gt(D->gt, (size_t)k, S, s); ++nf; }
    char *smp = strdup(column); int nv; char **vals = split(smp, ':', &nv);
    for (int i = 0; i < F->nk; ++i) {
        if (F->kjob && F->kjob[i] >= 0) continue;
        if (i == r->pl_idx) {
            if (c->pl_dropped || dev_rec) continue;
            if (nf++) fputc(':', LN);
            int printed = 0;
            for (int j = 0; j < ngn; ++j) {
                const int32_t v = D->opl[((size_t)k * ngmax + j) * S + s];
                if (v == BCFGPU_INT32_VECTOR_END) break;
                if (printed++) fputc(',', LN);
                if (v == BCFGPU_INT32_MISSING) fputc('.', LN); else fprintf(LN, "%d", v);
            }
            if (!printed) fputc('.', LN);
        } else if (i < nv && r->changed && is_numberR(fmtR, n_fmtR, F->keys[i], strlen(F->keys[i]))) {
            /* --device-alleles: the column is the input's own; the key goes through amap first (the sample part of the rewrite), then als_map */
            const size_t cap = BCFGPU_MAX_ALLELES * (strlen(vals[i]) + 2) + 8;
            obuf_t ob = { malloc(cap), 0, cap };
            constrained_numberR(&ob, vals[i], r->amap, r->nals);
            if (nf++) fputc(':', LN);
            if (nn != r->nals) print_numberR(ob.p, c->als_map, r->nals, nn); else fputs(ob.p, LN);
            free(ob.p);
        } else if (i < nv && nn != r->nals && is_numberR(fmtR, n_fmtR, F->keys[i], strlen(F->keys[i]))) {
            if (nf++) fputc(':', LN);
            print_numberR(vals[i], c->als_map, r->nals, nn);
        } else fprintf(LN, "%s%s", nf++ ? ":" : "", i < nv ? vals[i] : ".");
    }
    if (F->called && D->gp) {
        if (nf++) fputc(':', LN);
        int printed = 0;
        for (int j = 0; j < ngn; ++j) {
            uint32_t bits; memcpy(&bits, &D->gp[((size_t)k * ngmax + j) * S + s], 4);
            if (bits == 0x7F800002u) break;
            if (printed++) fputc(',', LN);
            if (bits == 0x7F800001u) fputc('.', LN); else fprintf(LN, "%g", (double)D->gp[((size_t)k * ngmax + j) * S + s]);
        }
        if (!printed) fputc('.', LN);
    }
    if (F->called && D->gq) {
        const int32_t v = D->gq[(size_t)k * S + s];
        if (v == BCFGPU_INT32_MISSING) fputs(":.", LN); else fprintf(LN, ":%d", v);
    }
    free(vals); free(smp);
}
typedef struct { char *dst; size_t len; } cursor_t;
static void put(cursor_t *c, const void *src, uint64_t b0, uint64_t b1) { memcpy(c->dst + c->len, (const char *)src + b0, (size_t)(b1 - b0)); c->len += (size_t)(b1 - b0); }
/* --device-records: the record's per-sample part: the device's blocks and the host's (made here from the sample text behind the
 * head, at head_end of the stream), in the FORMAT column's order */
static void splice_record(writer_t *W, int k, const fmt_t *F, long head_end)
{
    const rec_t *r = &W->R->rec[k]; const blocks_t *B = W->B; const int *kjob = F->kjob, nk = F->nk, with_gp = F->called && W->D->gp;
    end_head();
    int nhost = 0; size_t kend[64];
    if (F->host_keys > 0) {
        char *hf = malloc(strlen(r->fld[8]) + 8), *o = hf;              /* the host's keys as a FORMAT column of their own */
        for (int i = 0; i < nk; ++i) if (i != r->pl_idx && !(kjob && kjob[i] >= 0)) o += sprintf(o, "%s%s", o > hf ? ":" : "", F->keys[i]);
        if (with_gp) o += sprintf(o, "%sGP", o > hf ? ":" : "");
        if ((nhost = vio_encode_keys(W->hdr, hf, ln_buf + head_end, W->M->S, &W->hblk, &W->hblk_cap, kend)) != F->host_keys) DIE("%s\n", nhost < 0 ? vio_error() : "FORMAT keys lost on the way");
        free(hf);
    }
    const uint64_t *ko = B->koff + (size_t)k * BCFGPU_CALL_BCF_NKEYS, *poff = B->poff;
    size_t need = (size_t)(ko[BCFGPU_CALL_BCF_NKEYS] - ko[0]) + (nhost ? kend[nhost - 1] : 0);
    for (int i = 0; kjob && i < nk; ++i) if (kjob[i] >= 0) need += (size_t)(poff[kjob[i] + 1] - poff[kjob[i]]);
    if (need > W->iblk_cap) { W->iblk_cap = need * 2 + 256; W->iblk = realloc(W->iblk, W->iblk_cap); if (!W->iblk) DIE("out of memory\n"); }
    cursor_t cur = { W->iblk, 0 }; int hk = 0;
    put(&cur, B->kblk, ko[BCFGPU_CALL_BCF_GT], ko[BCFGPU_CALL_BCF_GT + 1]);
    for (int i = 0; i < nk + with_gp; ++i) {                    /* (GP, the host's, comes behind the input's keys) */
        if (i == r->pl_idx) put(&cur, B->kblk, ko[BCFGPU_CALL_BCF_PL], ko[BCFGPU_CALL_BCF_PL + 1]);
        else if (i < nk && kjob && kjob[i] >= 0) put(&cur, B->pblk, poff[kjob[i]], poff[kjob[i] + 1]);
        else { put(&cur, W->hblk, hk ? kend[hk - 1] : 0, kend[hk]); ++hk; }
    }
    put(&cur, B->kblk, ko[BCFGPU_CALL_BCF_GQ], ko[BCFGPU_CALL_BCF_GQ + 1]);
    if (vio_write_record_indiv(W->fout, W->hdr, ln_buf, W->iblk, cur.len)) DIE("%s\n", vio_error());
    rewind(LN);
}
/* record k as mcall.c:1627-1681 leaves it; gv_min_dp: the MinDP of a reference record outside the -g ranges, or 0 */
static void write_record(writer_t *W, int k, int gv_min_dp)
{
    const opt_t *o = W->o; const recs_t *R = W->R; const dev_t *D = W->D;
    const rec_t *r = &R->rec[k]; const bcfgpu_call_site *c = &D->cs[k];
    const int nn = c->nals_new, S = W->M->S, dev_rec = o->dev_rec;
    fprintf(LN, "%s\t%s\t%s\t%s\t", r->fld[0], r->fld[1], r->fld[2], r->fld[3]);
    print_alt(r, c);
    if (c->qual_missing) fputs("\t.", LN); else fprintf(LN, "\t%g", (double)c->qual);
    fprintf(LN, "\t%s\t", r->fld[6]);
    print_info(r, c, gv_min_dp);
    /* FORMAT: GT first, PL trimmed or dropped, the rest as it came */
    fmt_t F; char *fmt = strdup(r->fld[8]); F.keys = split(fmt, ':', &F.nk);
    F.called = nn > 1 && c->ret > 0;                           /* mcall_call_genotypes ran: GP and GQ exist (mcall.c:1618-1623) */
    /* --device-records: GT, PL and GQ are blocks already; the sample text holds the other keys alone (host_keys of them) */
    F.kjob = o->dev_keys && r->kjob && F.nk == r->nkjob ? r->kjob : NULL;     /* the keys whose blocks the device made */
    F.host_keys = dev_rec ? F.nk - 1 + (F.called && D->gp) : 0;
    for (int i = 0; F.kjob && i < F.nk; ++i) F.host_keys -= F.kjob[i] >= 0;
    const int text_ready = o->dev_text && W->B->toff[k + 1] > W->B->toff[k];     /* --device-text: the sample columns came from the device */
    const int want_text = !text_ready && (!dev_rec || F.host_keys > 0);
    if (dev_rec) W->B->n_phost += F.host_keys;
    if (o->text_given && !text_ready) ++W->B->n_thost;
    char **smp_fld = r->fld + 9;                               /* the input's sample columns */
    if (o->dev_in && want_text) {                            /* ... which become text here, for a record that is written */
        int ns;
        if (vio_indiv_text(W->hdr, R->ibuf + r->ioff, r->ilen, r->n_fmt, W->M->S_in, &W->smp_text, &W->smp_cap)) DIE("%s\n", vio_error());
        smp_fld = split(W->smp_text + 1, '\t', &ns);
        if (ns != W->M->S_in) DIE("malformed VCF\n");
    } else if (o->dev_parse && want_text) {                    /* --device-parse: the columns' text is split here, for a record that is written */
        int ns;
        if (r->ilen + 1 > W->smp_cap) { W->smp_cap = (r->ilen + 1) * 2; W->smp_text = realloc(W->smp_text, W->smp_cap); if (!W->smp_text) DIE("out of memory\n"); }
        memcpy(W->smp_text, R->ibuf + r->ioff, r->ilen); W->smp_text[r->ilen] = 0;
        smp_fld = split(W->smp_text + 1, '\t', &ns);
        if (ns != W->M->S_in) DIE("malformed VCF\n");
    }
    fputs("\tGT", LN);
    for (int i = 0; i < F.nk; ++i) if (i != r->pl_idx || !c->pl_dropped) fprintf(LN, ":%s", F.keys[i]);
    if (F.called && D->d_gp) fputs(":GP", LN);
    if (F.called && D->d_gq) fputs(":GQ", LN);
    const long head_end = dev_rec || text_ready ? end_head() : 0;      /* the head ends here; the other keys' sample text follows it in the stream */
    for (int s = 0; s < S && want_text; ++s) print_sample_text(W, k, &F, smp_fld[W->M->col[s]], s);
    if (text_ready) {                                         /* head and ready columns to the writer */
        if (vio_write_record_text(W->fout, W->hdr, ln_buf, W->B->tblk + W->B->toff[k], (size_t)(W->B->toff[k + 1] - W->B->toff[k]))) DIE("%s\n", vio_error());
        rewind(LN);
    } else if (dev_rec) splice_record(W, k, &F, head_end); else end_record(W->fout, W->hdr);
    free(F.keys); free(fmt);
    if ((o->dev_in || o->dev_parse) && want_text) free(smp_fld);
}
static void write_records(writer_t *W)
{
    const opt_t *o = W->o; const gvcf_t *G = W->G; const bcfgpu_call_site *cs = W->D->cs;
    const int n_out = cals ? n_events : W->R->n;
    for (int ev = 0; ev < n_out; ++ev) {
        if (cals && events[ev].is_missed) { write_missed_target(W, &tgt[events[ev].tgt]); continue; }
        const int k = cals ? events[ev].tgt : ev;
        if (cs[k].ret == -2 || (o->varonly && cs[k].ret == 0) || cs[k].ret < 0) continue;
        int gv_min_dp = 0;
        if (o->gv_n) {
            const int w = G->w[k], b = G->blk[w];
            if (b >= 0) {                                        /* inside a block: one line when the block ends */
                if (G->block[b].last_site == w) write_block_line(W, k, b);
                continue;
            }
            if (cs[k].ret == 1) gv_min_dp = G->min[w];             /* a reference record outside the ranges keeps MinDP (gvcf.c:221-222) */
        }
        write_record(W, k, gv_min_dp);
    }
}

int main(int argc, char **argv)
{
    opt_t o; ploidy_t P; smap_t M; recs_t R; hplanes_t H; dev_t D; blocks_t B; gvcf_t G; vio_hdr *hdr;
    if (parse_options(argc, argv, &o)) return 2;
    load_ploidy(&o, &P);
    vio_file *fin = open_input(&o, &hdr);
    const double t0 = now_s();
    for (int i = 0; i < vio_hdr_nlines(hdr); ++i) header_line(vio_hdr_line(hdr, i));
    map_samples(&o, &P, hdr, &M);
    read_records(&o, &P, &M, fin, hdr, &R);
    const double t_read = now_s() - t0;
    flush_last_targets(&R);
    if (M.S <= 0) DIE("no samples\n");
    read_groups(&o, &M);
    R.namax = 1;
    for (int k = 0; k < R.n; ++k) if (R.rec[k].nals > R.namax) R.namax = R.rec[k].nals;
    const double t1 = now_s();
    build_planes(&o, &M, &R, &H);
    const double t_planes = now_s() - t1, t2 = now_s();
    call_on_device(&o, &P, &M, &R, &H, &D);
    double t_dev = now_s() - t2, t_enc = 0.;
    const double t3 = now_s();
    output_header(&o, &M, hdr);
    memset(&B, 0, sizeof B); memset(&G, 0, sizeof G);
    if (o.dev_rec) {
        const double te = now_s();
        encode_call_blocks(&o, &R, &D, hdr, &B);
        if (o.dev_keys) encode_key_blocks(&o, &M, &R, &H, &D, hdr, &B);
        free(B.emit);
        t_enc = now_s() - te;                                    /* a device stage: counted there, not under writing */
    }
    if (o.dev_text) {
        const double te = now_s();
        if (o.dev_parse) rewrite_text_columns(&o, &M, &R, &D, &B); else encode_text_columns(&o, &M, &R, &D, &B);
        t_enc = now_s() - te;
    }
    vio_file *fout = vio_open_write(o.out_path, o.out_mode);
    if (!fout || vio_write_hdr(fout, hdr)) DIE("%s\n", vio_error());
    open_record_stream();
    if (o.gv_n) gvcf_blocks(&o, &M, &R, &D, &G);
    writer_t W; memset(&W, 0, sizeof W);
    W.o = &o; W.M = &M; W.R = &R; W.D = &D; W.B = &B; W.G = &G; W.fout = fout; W.hdr = hdr;
    write_records(&W);
    if (vio_close(fout)) DIE("%s\n", vio_error());
    const double t_write = now_s() - t3 - t_enc; t_dev += t_enc;
    if (o.want_timing) fprintf(stderr, "[bcfgpu_call] seconds: reading records %.3f, building the planes on the host %.3f, uploads and device stages %.3f, writing records %.3f\n", t_read, t_planes, t_dev, t_write);
    if (o.want_timing) fprintf(stderr, "[bcfgpu_call] device input: %d records' planes decoded on the device\n", o.dev_in ? R.n : 0);
    if (o.want_timing) fprintf(stderr, "[bcfgpu_call] device records: %d records' FORMAT blocks encoded on the device\n", B.n_enc);
    if (o.want_timing && o.parse_given) fprintf(stderr, "[bcfgpu_call] device parse: %d records' planes parsed on the device\n", o.dev_parse ? R.n : 0);
    if (o.want_timing && o.als_given) fprintf(stderr, "[bcfgpu_call] device alleles: %d records' planes constrained on the device, %d taken as they were\n", o.dev_als ? R.n_changed : 0, o.dev_als ? R.n - R.n_changed : 0);
    if (o.want_timing && o.keys_given) fprintf(stderr, "[bcfgpu_call] device keys: %ld pass-through key blocks made on the device, %ld on the host\n", B.n_pjob, B.n_phost);
    if (o.want_timing && o.text_given) fprintf(stderr, "[bcfgpu_call] device text: %ld records' sample columns formatted on the device, %ld on the host\n", B.n_tdev, B.n_thost);
    bcfgpu_destroy(D.ctx);
    return 0;
}
