/*  bcfgpu_sam.c -- `bcftools mpileup` over SAM / BAM files with every stage of the path on the device, in plain C over the
 *  C-ABI of include/bcfgpu.h (SNP and indel records).
 *
 *      bcfgpu_sam [options] -f ref.fa [-r CHR[:BEG[-END]],... | -R FILE] [-t [^]REG,... | -T [^]FILE] [-b FILE] file.sam|file.bam [...]         (mpileup's own spelling, mpileup.c:952-1003)
 *      bcfgpu_sam [options] ref.fa contig beg end file.sam|file.bam [...]                       (beg, end 1-based inclusive)
 *      options: -a TAG,..  --gvcf INT,..  -O v|z|u|b  -o FILE  -d INT  -s LIST  -S FILE  -G FILE  --ignore-RG
 *               -B  -E  -A  -q INT  -Q INT  -C INT  --ff INT  --rf INT  -I -o INT -e INT -h INT -m INT -F FLOAT -p -L INT   (as `bcftools mpileup`)
 *               --tile COLUMNS  columns per device tile (default 16384);  --gpus N  region shards, a process per shard
 *               --prefetch  the next tile's reads go to the device (bcfgpu_pool_stage, from page-locked buffers) while the device
 *                           stages of the current tile run; the same output
 *               --device-records  with -O u|b: the per-sample part of every SNP and indel record is encoded as BCF2 on the device
 *                           (bcfgpu_mplp_encode_bcf) and comes to the host as bytes instead of planes; the same output
 *               --device-text  with -O v|z: the sample columns of every SNP and indel record are formatted as VCF text on the device
 *                           (bcfgpu_mplp_encode_vcf) and come to the host as bytes instead of planes; the same output
 *               --list-samples: print "sample <TAB> reads entering the pileup <TAB> files" and stop (no device needed)
 *
 *  A region is streamed through in TILES: the files are read in step with the tiles -- a position-sorted file no
 *  further than the tile's, and in the end the region's, last column -- a read stays in host memory while it can still cover a
 *  column, and what the device holds at any time is one tile's reads and columns.  Memory is bounded by the tile, not by the
 *  region (mpileup_reg() walks column by column with the iterator's buffer, mpileup.c:327-367); several regions run one after the
 *  other (mpileup.c:652-683).
 *
 *  What stays on the host is what mpileup.c and htslib's pileup do before any arithmetic: parsing (SAM text; BAM = BGZF +
 *  binary records, inflated block by block), the read -> sample map of bam_sample.c (@RG SM, RG:Z tags, -s/-S/-G), the read
 *  filters of mplp_func (mpileup.c:183-246: unmapped, --rf/--ff flags, reads of dropped read groups, -q, orphans), the
 *  iterator's per-file depth cap (bcfgpu_depth_cap_push, its buffer carried from tile to tile) and the pairing of overlapping
 *  mates (htslib overlap_push).  Then per tile, each a call on the flat read pool:
 *      bcfgpu_pool_upload          the tile's reads to HBM, once (--prefetch: bcfgpu_pool_stage under the tile before, then
 *                                  bcfgpu_pool_adopt -- the read callback running ahead of the column loop, mpileup.c:183-246)
 *      bcfgpu_pool_baq             BAQ (sam_prob_realn, mpileup.c:234)
 *      bcfgpu_pool_overlap_tweak   mate-overlap qualities (bam_mplp_init_overlaps, mpileup.c:640)
 *      bcfgpu_pool_pileup          the pileup columns of the tile, built in HBM
 *      bcfgpu_mpileup              bcf_call_glfgen x samples + bcf_call_combine per column (mpileup.c:343-347)
 *  and for the columns where some read is followed by an indel (mpileup.c:354-365):
 *      bcfgpu_gap_prep_tile (bcf_call_gap_prep on the candidate columns, in HBM) -> bcfgpu_mpileup on its indel tile
 *  with -C INT: bcfgpu_pool_baq + bcfgpu_pool_cap_mapq on every batch of reads as it comes off the files (mpileup.c:234-241),
 *  with --device-records: bcfgpu_mplp_encode_bcf on the planes of both passes, the writer then frames the bytes (vio_write_record_indiv),
 *  with --device-text: bcfgpu_mplp_encode_vcf on them, the writer then puts the bytes behind the head (vio_write_record_text),
 *  with --gvcf: bcfgpu_gvcf_blocks per tile, the block that reaches a tile's end joined with the next tile's first (gvcf.c:88-226);
 *  and the record loop writes what bcf_call2bcf (bam2bcf.c:756-906) puts in the record, in its order, under mpileup's header
 *  (mpileup.c:510-602), as VCF, bgzipped VCF or BCF (host/vcfio.c).  tests/test_c_host.py compares the whole output with the
 *  reference's goldens test/mpileup/mpileup.{1..11}.out, mpileup-SCR.out, indel-AD.1.out -- one tile and many.
 *  Not here: CRAM input, index files (a region far into a file is reached by reading up to it);
 *  a sample fed by several files has its reads merged by position (the reference appends file after file: same
 *  records unless a cell passes 255 usable reads, where errmod_cal's draw then meets the reads in another order).
 *
 *  How the file reads.  The command line is one struct (opt_t O, filled by parse_options() alone), the run's output, counters and
 *  timers another (RUN).  main() is the list of the run's stages over a job_t:
 *      parse_options -> input_files (positional + -b) -> regions (-r, -R, CONTIG BEG END) -> open_inputs (headers -> samples,
 *      ##contig, the all-contigs default) -> shard_or_device (--gpus: the parent of the shards ends here) -> write_header ->
 *      tile_loop_init -> run_region per region -> report
 *  run_region()'s tile loop:  read_batch (the files, -C, the depth cap, into the live windows) -> fill_pool -> tile_submit, or the
 *  flush of a tile without reads -> retire_window.  tile_submit() prepares the tile on the host (tile_prepare) and, at once or one
 *  tile later (--prefetch), runs tile_device(), the list of the device stages over the tile's results (tile_out_t):
 *      tile_pileup -> record_rule_columns -> indel_candidates -> errmod_plan -> mpileup_passes -> gvcf_tile -> record_rule_snps ->
 *      encode_tile -> emit_submit
 *  and one writer thread turns the results into records (emit_tile).  Which column gets a record is written down once, in the
 *  arrays the record_rule_* stages fill (see tile_out_t).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <stdint.h>
#include <stddef.h>
#include <ctype.h>
#include <math.h>
#include <zlib.h>
#include <spawn.h>
#include <unistd.h>
#include <sys/types.h>
#include <sys/wait.h>
#include <fcntl.h>
#include <signal.h>
#include <pthread.h>
#include <sys/syscall.h>
extern long syscall(long number, ...);       /* (unistd.h keeps it back under -std=c99 -D_POSIX_C_SOURCE) */
#include "bcfgpu.h"
#include "vcfio.h"
#include "drv.h"

/* ---- what the command line sets.  One instance, O, filled by parse_options() (with the readers of its lists: target_spec,
 * target_file, add_samples, add_readgroups) and by nothing else; every stage, the parser threads and the record writer only read it. ---- */
typedef struct { char **key, **val; int n; } smap_t;                        /* a small string map; lookups are per @RG line */
typedef struct { char *chrom; long beg, end; } target_t;                    /* 0-based inclusive [beg, end]; end < 0: to the end of the sequence */
typedef struct {
    /* what to run on: -f, -r, -R, -b; pos_region: CONTIG BEG END of the five-argument spelling, else NULLs */
    const char *ref_path, *reg_arg, *reg_file, *file_list, *pos_region[3];
    target_t *target; int n_target, target_incl;                            /* -t / -T; target_incl 0: the ^ form */
    /* the read -> sample map (bam_sample.c) */
    int ignore_rg;                                                          /* --ignore-RG */
    int have_samples, sample_logic; smap_t samples;                         /* -s/-S: input sample -> output name; 1 include, 0 exclude */
    int have_rgs, rg_logic; smap_t rgs;                                     /* -G: "id" | "id\tfile" | "*\tfile" -> name or "\t" (keep) */
    /* the read filters of mplp_func (mpileup.c:183-246) and what is done to a read before the pileup */
    int rflag_require, rflag_filter, min_mq, keep_orphans;                  /* --rf, --ff, -q, -A */
    int no_overlaps, illumina13;                                            /* -x: the mates' overlaps are left alone (mpileup.c:1005); -6 (mpileup.c:216-221) */
    int max_depth, baq_flag, min_baseQ, cap_thres;                          /* -d; -B / -E; -Q; -C (mpileup.c:937-950) */
    int no_indels, max_indel_depth, openQ, extQ, tandemQ, min_support, per_sample_flt; double min_frac;    /* -I -L -o -e -h -m -p -F */
    /* the output */
    char out_mode; const char *out_path;                                    /* -O, -o / --output */
    int fmt_flag;                                                           /* mpileup's default annotations + -a (+ FORMAT/DP with --gvcf) */
    int32_t gv_range[16]; int gv_n;                                         /* --gvcf INT,.. (gvcf.c:44-67) */
    /* how to run */
    int tile_cols, n_gpus, shard, list_only, want_timing;                   /* --tile; --gpus N, --shard K: this is shard K; --list-samples; --timing */
    int prefetch, device_records, device_text;                              /* the options as given */
    /* derived, once the last option is read */
    int dr_on, dt_on;                       /* --device-records on a BCF output (-O u|b); --device-text on a text output (-O v|z) */
    int defer_mq_filters;                   /* -C: sam_cap_mapq comes between the flag filters and the -q / orphan filters (mpileup.c:234-241) */
} opt_t;
static opt_t O;
#define DEV_ON (O.dr_on || O.dt_on)         /* the planes stay in HBM, the records' per-sample part comes as bytes */

/* ---- the state of the run.  fout, hdr: set by write_header() (or by the parent of the shards) on the main thread before the first
 * tile is handed over, then the record writer's alone until emit_wait() / emit_finish().  The counters and timers each have one
 * writing thread, and report() reads them after emit_finish() has joined the writer:
 *     main thread:    n_reads, n_cols, n_tiles, tot_entries, tot_pairs, n_wide_cells, t_read, t_pool, t_dev, t_adopt
 *     record writer:  n_dev_records, n_dev_text, t_emit ---- */
static struct {
    vio_file *fout; vio_hdr *hdr;
    int32_t dr_key[BCFGPU_BCF_NKEYS];                                        /* --device-records: the FORMAT keys' indices in the header's dictionary (write_header) */
    unsigned long long n_reads, n_cols; int n_tiles;                         /* what the report's summary line counts */
    unsigned long long tot_entries, tot_pairs;                               /* pileup entries; overlapping mate pairs */
    unsigned long long n_wide_cells;                                         /* cells of more than 255 usable reads left to the first-255 rule */
    unsigned long long n_dev_records, n_dev_text;                            /* records written with a block / with sample columns from the device */
    /* --timing: where the wall time of a run goes (seconds): reading and parsing the files, building a tile's pool, the device
     * stages of a tile (every call up to the records' planes on the host), writing the records; with --prefetch the wait inside
     * bcfgpu_pool_adopt (what of the next tile's copy the current tile's stages did not cover) */
    double t_read, t_pool, t_dev, t_emit, t_adopt;
} RUN;

typedef struct {
    int n, cap;                                   /* reads */
    int32_t *pos, *lq, *flag, *ncig, *cig_off, *seq_off, *smpl, *file, *end, *mpos, *isize, *rnext_same;
    uint8_t *mapq, *has_zq;
    char **qname;
    uint32_t *cig; size_t ncigs, cigcap;
    uint8_t *seq16, *qual, *zq; size_t nbase, basecap;
    int pinned;                                   /* the arrays are page-locked (bcfgpu_host_alloc): --prefetch copies from them beside kernels */
} pool_t;

static void *grow(void *p, size_t n) { p = realloc(p, n ? n : 1); if (!p) DIE("out of memory\n"); return p; }
/* a pool's array of `used` bytes made n bytes long */
static void *pool_grow(const pool_t *P, void *p, size_t used, size_t n)
{
    if (!P->pinned) return grow(p, n);
    void *q = NULL;
    if (bcfgpu_host_alloc(n ? n : 1, &q)) DIE("%s\n", bcfgpu_last_error());
    if (p) { memcpy(q, p, used); bcfgpu_host_free(p); }
    return q;
}

static int nt16_of(char c)
{
    static const char *codes = "=ACMGRSVTWYHKDBN";
    const char *q = strchr(codes, toupper((unsigned char)c));
    return (q && *q) ? (int)(q - codes) : 15;
}

static char *read_contig(const char *path, const char *name, int *len)
{
    FILE *f = fopen(path, "r");
    if (!f) DIE("cannot open %s\n", path);
    char line[1 << 16], *seq = NULL;
    size_t n = 0, cap = 0;
    int in = 0;
    while (fgets(line, sizeof line, f)) {
        if (line[0] == '>') {
            char *e = line + 1;
            while (*e && !isspace((unsigned char)*e)) ++e;
            *e = 0;
            in = strcmp(line + 1, name) == 0;
            continue;
        }
        if (!in) continue;
        size_t l = strlen(line);
        while (l && isspace((unsigned char)line[l - 1])) --l;
        if (n + l + 1 > cap) { cap = (n + l + 1) * 2; seq = grow(seq, cap); }
        memcpy(seq + n, line, l); n += l;
    }
    fclose(f);
    if (!seq) DIE("contig %s not found in %s\n", name, path);
    seq[n] = 0; *len = (int)n;
    return seq;
}

/* ---- which reads belong to which output sample: bam_sample.c (bam_smpl_add_bam, bam_smpl_get_sample_id, -s/-S/-G) ---- */
static const char *smap_get(const smap_t *m, const char *k) { for (int i = 0; i < m->n; ++i) if (!strcmp(m->key[i], k)) return m->val[i]; return NULL; }
static void smap_set(smap_t *m, const char *k, const char *v)
{
    m->key = grow(m->key, (size_t)(m->n + 1) * sizeof *m->key); m->val = grow(m->val, (size_t)(m->n + 1) * sizeof *m->val);
    m->key[m->n] = strdup(k); m->val[m->n++] = strdup(v);
}
typedef struct { const char *fname; int default_idx, nrg; char **rg; int *rg_smpl; } sfile_t;
static struct { int nsmpl; char **smpl; } SM;                              /* output samples, in order of first appearance (open_inputs) */

static int rg_find(const sfile_t *f, const char *id) { for (int i = 0; i < f->nrg; ++i) if (!strcmp(f->rg[i], id)) return i; return -1; }
static int smpl_find(const char *name) { for (int i = 0; i < SM.nsmpl; ++i) if (!strcmp(SM.smpl[i], name)) return i; return -1; }

/* bsmpl_add_readgroup: name NULL = the read group is known but its reads are dropped; id "*" = the whole file */
static void rg_add(sfile_t *f, const char *id, const char *name)
{
    int is = -1;
    if (name && (is = smpl_find(name)) < 0) {
        SM.smpl = grow(SM.smpl, (size_t)(SM.nsmpl + 1) * sizeof *SM.smpl);
        SM.smpl[is = SM.nsmpl++] = strdup(name);
    }
    if (!strcmp(id, "*")) { f->default_idx = is; return; }
    if (rg_find(f, id) >= 0) return;                                        /* a repeated @RG ID: the first one counts */
    f->rg = grow(f->rg, (size_t)(f->nrg + 1) * sizeof *f->rg); f->rg_smpl = grow(f->rg_smpl, (size_t)(f->nrg + 1) * sizeof *f->rg_smpl);
    f->rg[f->nrg] = strdup(id); f->rg_smpl[f->nrg++] = is;
}
/* bsmpl_keep_readgroup: the -G list, most specific entry first; may rename the sample */
static int rg_keep(const sfile_t *f, const char *id, const char **name)
{
    char key[4096];
    const char *v = smap_get(&O.rgs, id);
    if (!v) { snprintf(key, sizeof key, "%s\t%s", id, f->fname); v = smap_get(&O.rgs, key); }
    if (!v) { snprintf(key, sizeof key, "*\t%s", f->fname); v = smap_get(&O.rgs, key); }
    if ((!v && O.rg_logic) || (v && !O.rg_logic)) return 0;
    if (v && v[0] != '\t') *name = v;
    return 1;
}
/* one whitespace-delimited field with backslash escapes (bam_smpl_add_samples / bam_smpl_add_readgroups) */
static const char *next_field(const char *p, char *out, size_t cap)
{
    size_t n = 0; int esc = 0;
    while (*p && isspace((unsigned char)*p)) ++p;
    for (; *p; ++p) {
        if (*p == '\\' && !esc) { esc = 1; continue; }
        if (isspace((unsigned char)*p) && !esc) break;
        if (n + 1 < cap) out[n++] = *p;
        esc = 0;
    }
    out[n] = 0;
    return p;
}
/* hts_readlist: the rows of a file, or the comma-separated items of the argument */
static char **read_list(const char *arg, int is_file, int *n)
{
    char **rows = NULL; *n = 0;
    char *text = NULL;
    if (is_file) {
        FILE *f = fopen(arg, "r");
        if (!f) DIE("cannot open %s\n", arg);
        size_t len = 0, cap = 0; int c;
        while ((c = fgetc(f)) != EOF) { if (len + 2 > cap) { cap = cap ? 2 * cap : 4096; text = grow(text, cap); } text[len++] = (char)c; }
        fclose(f);
        if (!text) return NULL;
        text[len] = 0;
    } else text = strdup(arg);
    for (char *t = strtok(text, is_file ? "\r\n" : ","); t; t = strtok(NULL, is_file ? "\r\n" : ",")) {
        rows = grow(rows, (size_t)(*n + 1) * sizeof *rows); rows[(*n)++] = strdup(t);
    }
    free(text);
    return rows;
}
static void add_samples(const char *list, int is_file)                     /* -s / -S */
{
    if (list[0] != '^') O.sample_logic = 1; else ++list;
    int n; char **rows = read_list(list, is_file, &n);
    if (!n) return;
    O.have_samples = 1;
    for (int i = 0; i < n; ++i) {
        char a[1024], b[1024];
        const char *p = next_field(rows[i], a, sizeof a);
        next_field(p, b, sizeof b);
        if (!smap_get(&O.samples, a)) smap_set(&O.samples, a, b[0] ? b : a);
        free(rows[i]);
    }
    free(rows);
}
static void add_readgroups(const char *list)                               /* -G: rows "ID", "ID SAMPLE" or "ID FILE SAMPLE" */
{
    if (list[0] != '^') O.rg_logic = 1; else ++list;
    int n; char **rows = read_list(list, 1, &n);
    if (!n) return;
    O.have_rgs = 1;
    for (int i = 0; i < n; ++i) {
        char a[1024], b[1024], c[1024], key[2100];
        const char *p = next_field(rows[i], a, sizeof a);
        p = next_field(p, b, sizeof b);
        next_field(p, c, sizeof c);
        const char *val = c[0] ? c : b[0] ? b : "\t";
        if (c[0]) snprintf(key, sizeof key, "%s\t%s", a, b); else snprintf(key, sizeof key, "%s", a);
        const char *old = smap_get(&O.rgs, key);
        if (!old) smap_set(&O.rgs, key, val);
        else if (strcmp(old, val)) DIE("Error: The read group \"%s\" was assigned to two different samples: \"%s\" and \"%s\"\n", key, old, val);
        free(rows[i]);
    }
    free(rows);
}
/* bam_smpl_add_bam over the header text; 0: no read of the file can be used, the file is dropped */
static int add_file(sfile_t *f, const char *fname, const char *hdr_text)
{
    memset(f, 0, sizeof *f);
    f->fname = fname; f->default_idx = -1;
    if (O.ignore_rg || !hdr_text || !hdr_text[0]) { rg_add(f, "*", fname); return 1; }
    int first_smpl = -1, nskipped = 0, n_file_smpl = 0;
    char **file_smpl = NULL;
    for (const char *line = hdr_text; line && *line; ) {
        const char *eol = strchr(line, '\n');
        const size_t len = eol ? (size_t)(eol - line) : strlen(line);
        if (len > 3 && !strncmp(line, "@RG", 3)) {
            char *l = malloc(len + 1); memcpy(l, line, len); l[len] = 0;
            if (len && l[len - 1] == '\r') l[len - 1] = 0;
            char *id = strstr(l, "\tID:"), *sm = strstr(l, "\tSM:");
            if (!id || !sm) { free(l); break; }                             /* the scan ends at an @RG without ID or SM */
            id += 4; sm += 4;
            id[strcspn(id, "\t")] = 0; sm[strcspn(sm, "\t")] = 0;
            if (!strcmp(id, "*") || !strcmp(id, "?")) DIE("Error: the read group IDs \"*\" and \"?\" have a special meaning: %s\n", fname);
            const char *name = sm;
            int accept = 1;
            if (O.have_samples) {
                const char *ren = smap_get(&O.samples, sm);
                if (!O.sample_logic) accept = ren ? 0 : 1;
                else if (!ren) accept = 0;
                else name = ren;
            }
            if (accept && O.have_rgs) accept = rg_keep(f, id, &name);
            if (accept) rg_add(f, id, name); else { rg_add(f, id, NULL); ++nskipped; }
            if (first_smpl < 0) first_smpl = smpl_find(name);
            int k; for (k = 0; k < n_file_smpl; ++k) if (!strcmp(file_smpl[k], name)) break;
            if (k == n_file_smpl) { file_smpl = grow(file_smpl, (size_t)(n_file_smpl + 1) * sizeof *file_smpl); file_smpl[n_file_smpl++] = strdup(name); }
            free(l);
        }
        line = eol ? eol + 1 : NULL;
    }
    for (int k = 0; k < n_file_smpl; ++k) free(file_smpl[k]);
    free(file_smpl);
    /* reads without a read group, or with one the header does not list */
    const char *null_name = NULL;
    int accept_null = 1;
    if (O.have_rgs && !rg_keep(f, "?", &null_name)) accept_null = 0;
    if (O.have_samples && first_smpl == -1) accept_null = 0;
    if (!accept_null && first_smpl == -1) return 0;
    if (!accept_null) return 1;
    if (n_file_smpl == 1 && !nskipped) { f->default_idx = first_smpl; return 1; }
    if (!null_name) null_name = first_smpl == -1 ? fname : SM.smpl[first_smpl];
    rg_add(f, "?", null_name);
    return 1;
}
static int sample_of(const sfile_t *f, const char *rg)                      /* bam_smpl_get_sample_id; rg NULL: no RG tag */
{
    if (f->default_idx >= 0) return f->default_idx;
    int i = rg_find(f, rg ? rg : "?");
    if (i < 0) i = rg_find(f, "?");
    return i < 0 ? -1 : f->rg_smpl[i];
}

/* ---- reading: SAM text or BAM; the read filters of mplp_func (mpileup.c:183-246) ---- */
/* -t / -T: the targets (mpileup.c:198-212, 330-335, 1033-1051): reads that overlap none of them never enter the pileup, columns outside
 * them give no record; a leading ^ turns the list into the columns to leave out (the reads are chosen as without it, as in the reference).
 * target_add, target_spec and target_file are parse_options' */
static void target_add(const char *chrom, size_t cl, long beg, long end)
{
    O.target = realloc(O.target, (size_t)(O.n_target + 1) * sizeof *O.target);
    O.target[O.n_target].chrom = strndup(chrom, cl); O.target[O.n_target].beg = beg; O.target[O.n_target].end = end; ++O.n_target;
}
static void target_spec(const char *spec)                                          /* CHR, CHR:POS, CHR:BEG-END (1-based) */
{
    const char *c = strrchr(spec, ':'); char *e = NULL;
    long a = c ? strtol(c + 1, &e, 10) : 0;
    if (!c || e == c + 1) { target_add(spec, strlen(spec), 0, -1); return; }
    const long b = *e == '-' ? (e[1] ? strtol(e + 1, NULL, 10) : 0) : a;
    target_add(spec, (size_t)(c - spec), a - 1, b ? b - 1 : -1);
}
static void target_file(const char *path)                                          /* CHROM <tab> POS [<tab> END], 1-based inclusive */
{
    FILE *f = fopen(path, "r");
    if (!f) { fprintf(stderr, "Could not read file \"%s\"\n", path); exit(1); }
    char ln[4096], c[1024]; long a, b;
    while (fgets(ln, sizeof ln, f)) {
        if (ln[0] == '#') continue;
        const int k = sscanf(ln, "%1023s %ld %ld", c, &a, &b);
        if (k >= 1) target_add(c, strlen(c), k >= 2 ? a - 1 : 0, k >= 3 ? b - 1 : k == 2 ? a - 1 : -1);
    }
    fclose(f);
}
/* does [beg, end] of `chrom` overlap a target?  *inside: it lies wholly inside one */
static int target_overlap(const char *chrom, long beg, long end, int *inside)
{
    int ov = 0;
    if (inside) *inside = 0;
    for (int i = 0; i < O.n_target; ++i) {
        if (strcmp(O.target[i].chrom, chrom)) continue;
        const long tb = O.target[i].beg, te = O.target[i].end < 0 ? (1L << 40) : O.target[i].end;
        if (beg <= te && end >= tb) { ov = 1; if (inside && beg >= tb && end <= te) *inside = 1; }
    }
    return ov;
}
static int target_keeps_read(const char *chrom, long beg, long end)                /* mpileup.c:198-212 */
{
    /* As the reference has it: a read goes on if it overlaps a listed stretch -- with the ^ form too (its "exclude only reads which are
     * fully contained" loop runs only when nothing overlaps, over no region, so a read clear of the list is dropped there as well). */
    return !O.n_target || target_overlap(chrom, beg, end, NULL);
}
/* a linear scan over the targets: asked once per column of a tile (record_rule_columns), and nowhere else */
static int target_keeps_column(const char *chrom, long pos)                        /* mpileup.c:330-335 */
{
    if (!O.n_target) return 1;
    const int ov = target_overlap(chrom, pos, pos, NULL);
    return O.target_incl ? ov : !ov;
}
/* the region being read: only reads that overlap it enter the pool, as htslib's region iterator hands them out.  Set by run_region()
 * before the region's parser threads start, read by them */
static int reg_beg = 0, reg_end = 0x7fffffff;

static void pool_add(pool_t *P, int file, int smpl, const char *qname, int flag, int pos, int mapq, int rnext_same, int mpos, int isize,
                     const uint32_t *cig, int ncig, int lq, const uint8_t *seq16, const uint8_t *qual)
{
    if (P->n == P->cap) {
        const size_t used = (size_t)P->cap, cap = used ? 2 * used : 1024;
        int32_t **i32[12] = { &P->pos, &P->lq, &P->flag, &P->ncig, &P->cig_off, &P->seq_off, &P->smpl, &P->file, &P->end, &P->mpos, &P->isize, &P->rnext_same };
        for (int a = 0; a < 12; ++a) *i32[a] = pool_grow(P, *i32[a], used * 4, cap * 4);
        P->mapq = pool_grow(P, P->mapq, used, cap); P->has_zq = pool_grow(P, P->has_zq, used, cap);
        P->qname = pool_grow(P, P->qname, used * sizeof *P->qname, cap * sizeof *P->qname);
        P->cap = (int)cap;
    }
    const int r = P->n++;
    P->qname[r] = (char *)qname;                       /* borrowed: the live window owns the name */
    P->flag[r] = flag; P->pos[r] = pos; P->mapq[r] = (uint8_t)mapq; P->smpl[r] = smpl; P->file[r] = file; P->has_zq[r] = 0;
    P->rnext_same[r] = rnext_same; P->mpos[r] = mpos; P->isize[r] = isize;
    P->cig_off[r] = (int32_t)P->ncigs; P->ncig[r] = ncig;
    if (P->ncigs + ncig + 1 > P->cigcap) { P->cigcap = (P->ncigs + ncig + 1) * 2; P->cig = pool_grow(P, P->cig, P->ncigs * 4, P->cigcap * 4); }
    int x = pos;
    for (int c = 0; c < ncig; ++c) {
        const int op = cig[c] & 15;
        P->cig[P->ncigs++] = cig[c];
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) x += (int)(cig[c] >> 4);
    }
    P->end[r] = x;
    P->lq[r] = lq; P->seq_off[r] = (int32_t)P->nbase;
    if (P->nbase + lq + 1 > P->basecap) {
        P->basecap = (P->nbase + lq + 1) * 2;
        P->seq16 = pool_grow(P, P->seq16, P->nbase, P->basecap); P->qual = pool_grow(P, P->qual, P->nbase, P->basecap); P->zq = pool_grow(P, P->zq, P->nbase, P->basecap);
    }
    memcpy(P->seq16 + P->nbase, seq16, (size_t)lq); memcpy(P->qual + P->nbase, qual, (size_t)lq); memset(P->zq + P->nbase, 0, (size_t)lq);
    P->nbase += lq;
}
static int read_passes(int flag, int mapq)
{
    if (flag & 4) return 0;
    if (O.rflag_require && !(O.rflag_require & flag)) return 0;
    if (O.rflag_filter && (O.rflag_filter & flag)) return 0;
    if (O.defer_mq_filters) return 1;
    if (mapq < O.min_mq) return 0;
    if (!O.keep_orphans && (flag & 1) && !(flag & 2)) return 0;
    return 1;
}
static void contig_line(vio_hdr *h, const char *name, int nlen, long length)
{
    char buf[1200]; snprintf(buf, sizeof buf, "##contig=<ID=%.*s,length=%ld>", nlen, name, length);
    vio_hdr_append(h, buf);
}

/* ---- streaming input: one reader per file (SAM text, or BAM = BGZF + binary records, SAM spec 4.2), reads handed out in file
 * order.  A read leaves the reader only if it is on the region's contig, overlaps the region, passes the flag filters of
 * mplp_func (mpileup.c:183-246) and belongs to an output sample; a position-sorted file is read no further than the region's
 * end (htslib's region iterator stops there too). ---- */
typedef struct {
    char *qname; int flag, pos, mapq, rnext_same, mpos, isize, ncig, lq, end, smpl;
    uint32_t *cig; uint8_t *seq16, *qual;
} lrec_t;
static void lrec_free(lrec_t *r) { if (r) { free(r->qname); free(r->cig); free(r->seq16); free(r->qual); free(r); } }

typedef struct {
    const char *path; FILE *fp; int is_bam, eof, done, seen_contig;
    z_stream zs; int zs_on; uint8_t *zin;                   /* BAM: the BGZF stream, inflated member after member */
    uint8_t *buf; size_t buf_n, buf_rd, buf_cap;            /* BAM: inflated bytes not yet consumed */
    int tid, n_ref; char **ref_name; int32_t *ref_len;      /* BAM: the reference dictionary; tid = the region's contig */
    char *text;                                             /* the header text ('@' lines) */
    char *line; size_t line_cap; int have_line;             /* SAM: one text line of look-ahead */
    lrec_t *pend;                                           /* the next read parsed, not yet handed on (the parsing side's) */
    /* the consuming side: parsed reads wait in a ring (filled by a parsing thread, below); head = the next read, not yet taken */
    lrec_t *head; int drained;
    lrec_t **q; int q_rd, q_n, q_done;                      /* ring of RQ_CAP reads; q_done: the parsing side is through with the region */
    struct parser *owner;
} reader_t;

static int32_t le32(const uint8_t *p) { return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24); }

/* at least `need` inflated bytes at buf + buf_rd; 0 at the end of the file */
static int bz_fill(reader_t *r, size_t need)
{
    if (r->buf_n - r->buf_rd >= need) return 1;
    if (r->buf_rd) { memmove(r->buf, r->buf + r->buf_rd, r->buf_n - r->buf_rd); r->buf_n -= r->buf_rd; r->buf_rd = 0; }
    if (r->buf_cap < need + (1 << 16)) { r->buf_cap = need + (1 << 17); r->buf = grow(r->buf, r->buf_cap); }
    while (r->buf_n < need) {
        if (r->zs.avail_in == 0) {
            if (r->eof) break;
            const size_t got = fread(r->zin, 1, 1 << 16, r->fp);
            if (!got) { r->eof = 1; break; }
            r->zs.next_in = r->zin; r->zs.avail_in = (uInt)got;
        }
        r->zs.next_out = r->buf + r->buf_n; r->zs.avail_out = (uInt)(r->buf_cap - r->buf_n);
        const int rc = inflate(&r->zs, Z_NO_FLUSH);
        r->buf_n = r->buf_cap - r->zs.avail_out;
        if (rc == Z_STREAM_END) { if (inflateReset(&r->zs) != Z_OK) DIE("zlib: inflateReset failed\n"); }     /* the next BGZF block */
        else if (rc != Z_OK && rc != Z_BUF_ERROR) DIE("%s: corrupt BGZF block\n", r->path);
    }
    return r->buf_n - r->buf_rd >= need;
}

static void reader_close(reader_t *r)
{
    if (r->fp) fclose(r->fp);
    if (r->zs_on) inflateEnd(&r->zs);
    free(r->zin); free(r->buf); free(r->text); free(r->line);
    for (int i = 0; i < r->n_ref; ++i) free(r->ref_name[i]);
    free(r->ref_name); free(r->ref_len);
    lrec_free(r->pend);
    const char *p = r->path;
    memset(r, 0, sizeof *r); r->path = p;
}

/* opens the file and reads its header (r->text; BAM: the reference dictionary too) */
static void reader_open(reader_t *r, const char *path)
{
    memset(r, 0, sizeof *r);
    r->path = path; r->tid = -1;
    r->fp = fopen(path, "rb");
    if (!r->fp) DIE("cannot open %s\n", path);
    const int c0 = fgetc(r->fp), c1 = fgetc(r->fp);
    rewind(r->fp);
    if (c0 == 0x1f && c1 == 0x8b) {
        r->is_bam = 1; r->zin = grow(NULL, 1 << 16);
        if (inflateInit2(&r->zs, 15 + 16) != Z_OK) DIE("zlib: inflateInit2 failed\n");
        r->zs_on = 1;
        if (!bz_fill(r, 12) || memcmp(r->buf + r->buf_rd, "BAM\1", 4)) DIE("%s: not a BAM file\n", path);
        const size_t l_text = (uint32_t)le32(r->buf + r->buf_rd + 4);
        if (!bz_fill(r, 12 + l_text)) DIE("%s: truncated BAM header\n", path);
        r->text = grow(NULL, l_text + 1); memcpy(r->text, r->buf + r->buf_rd + 8, l_text); r->text[l_text] = 0;
        r->n_ref = le32(r->buf + r->buf_rd + 8 + l_text);
        r->buf_rd += 12 + l_text;
        r->ref_name = grow(NULL, (size_t)(r->n_ref + 1) * sizeof *r->ref_name); r->ref_len = grow(NULL, (size_t)(r->n_ref + 1) * sizeof *r->ref_len);
        for (int i = 0; i < r->n_ref; ++i) {
            if (!bz_fill(r, 4)) DIE("%s: truncated BAM header\n", path);
            const int l_name = le32(r->buf + r->buf_rd);
            if (l_name < 1 || !bz_fill(r, 8 + (size_t)l_name)) DIE("%s: truncated BAM header\n", path);
            r->ref_name[i] = grow(NULL, (size_t)l_name + 1); memcpy(r->ref_name[i], r->buf + r->buf_rd + 4, (size_t)l_name); r->ref_name[i][l_name] = 0;
            r->ref_len[i] = le32(r->buf + r->buf_rd + 4 + l_name);
            r->buf_rd += 8 + (size_t)l_name;
        }
        return;
    }
    /* SAM text: the '@' lines; the first other line stays as look-ahead */
    size_t tl = 0, tcap = 0;
    ssize_t n;
    while ((n = getline(&r->line, &r->line_cap, r->fp)) > 0) {
        if (r->line[0] != '@') { r->have_line = 1; break; }
        if (tl + (size_t)n + 1 > tcap) { tcap = (tl + (size_t)n + 1) * 2; r->text = grow(r->text, tcap); }
        memcpy(r->text + tl, r->line, (size_t)n); tl += (size_t)n;
    }
    if (!r->text) r->text = grow(NULL, 1);
    r->text[tl] = 0;
}

/* the value of the RG:Z tag in a BAM record's auxiliary data (SAM spec 4.2.4), or NULL */
static const char *bam_aux_rg(const uint8_t *a, const uint8_t *end)
{
    while (a + 3 <= end) {
        const int is_rg = a[0] == 'R' && a[1] == 'G';
        const char t = (char)a[2];
        a += 3;
        size_t l;
        switch (t) {
        case 'A': case 'c': case 'C': l = 1; break;
        case 's': case 'S': l = 2; break;
        case 'i': case 'I': case 'f': l = 4; break;
        case 'Z': case 'H': if (is_rg && t == 'Z') return (const char *)a; l = strnlen((const char *)a, (size_t)(end - a)) + 1; break;
        case 'B': {
            if (a + 5 > end) return NULL;
            const char st = (char)a[0]; const size_t cnt = (uint32_t)le32(a + 1);
            l = 5 + cnt * (st == 'c' || st == 'C' ? 1 : st == 's' || st == 'S' ? 2 : 4); break;
        }
        default: return NULL;
        }
        a += l;
    }
    return NULL;
}

static int ref_span_end(int pos, const uint32_t *cig, int ncig)
{
    int e = pos;
    for (int c = 0; c < ncig; ++c) { const int op = cig[c] & 15; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) e += (int)(cig[c] >> 4); }
    return e;
}
/* [pos, endpos) against [lo, hi) (a read without a reference span counts as one base: bam_endpos) */
static int overlaps(int pos, int end, int lo, int hi) { if (end == pos) end = pos + 1; return pos < hi && end > lo; }

static lrec_t *lrec_new(const char *qname, int flag, int pos, int mapq, int rnext_same, int mpos, int isize, const uint32_t *cig, int ncig, int lq, int smpl)
{
    lrec_t *x = grow(NULL, sizeof *x);
    x->qname = strdup(qname); x->flag = flag; x->pos = pos; x->mapq = mapq; x->rnext_same = rnext_same; x->mpos = mpos; x->isize = isize;
    x->ncig = ncig; x->lq = lq; x->smpl = smpl;
    x->cig = grow(NULL, (size_t)(ncig + 1) * 4); memcpy(x->cig, cig, (size_t)ncig * 4);
    x->end = ref_span_end(pos, cig, ncig);
    x->seq16 = grow(NULL, (size_t)lq + 1); x->qual = grow(NULL, (size_t)lq + 1);
    return x;
}

/* the next read of the file that can enter the pileup of region [reg_beg, reg_end) of `contig`, into r->pend; r->done at the end */
static void reader_parse(reader_t *r, const char *contig, const sfile_t *sf)
{
    if (r->pend || r->done) return;
    uint32_t cig[4096];
    if (r->is_bam) {
        if (r->tid < 0) {
            for (int i = 0; i < r->n_ref; ++i) if (!strcmp(r->ref_name[i], contig)) r->tid = i;
            if (r->tid < 0) { r->done = 1; return; }
        }
        for (;;) {
            if (!bz_fill(r, 4)) { r->done = 1; return; }
            const size_t bs = (uint32_t)le32(r->buf + r->buf_rd);
            if (bs < 32 || !bz_fill(r, 4 + bs)) DIE("%s: truncated BAM record\n", r->path);
            const uint8_t *b = r->buf + r->buf_rd;
            r->buf_rd += 4 + bs;
            const int refid = le32(b + 4), pos = le32(b + 8), l_name = b[12], mapq = b[13];
            const int n_cig = b[16] | b[17] << 8, flag = b[18] | b[19] << 8, l_seq = le32(b + 20);
            const int next_ref = le32(b + 24), next_pos = le32(b + 28), tlen = le32(b + 32);
            if (refid == r->tid) r->seen_contig = 1;
            /* a position-sorted file: nothing of the region follows a read past its end, or the reads of the next contig */
            if (r->seen_contig && (refid != r->tid || pos >= reg_end)) { r->done = 1; return; }
            if (refid != r->tid || !read_passes(flag, mapq)) continue;
            if (n_cig > 4096) DIE("%s: CIGAR with more than 4096 operations\n", r->path);
            const uint8_t *cg = b + 36 + l_name, *sq = cg + 4 * (size_t)n_cig, *ql = sq + (l_seq + 1) / 2, *aux = ql + l_seq;
            if (aux > b + 4 + bs) DIE("%s: malformed BAM record\n", r->path);
            for (int c = 0; c < n_cig; ++c) cig[c] = (uint32_t)le32(cg + 4 * c);
            if (!overlaps(pos, ref_span_end(pos, cig, n_cig), reg_beg, reg_end)) continue;
            if (!target_keeps_read(contig, pos, ref_span_end(pos, cig, n_cig) - 1)) continue;
            const int smpl = sample_of(sf, bam_aux_rg(aux, b + 4 + bs));
            if (smpl < 0) continue;
            lrec_t *x = lrec_new((const char *)b + 36, flag, pos, mapq, next_ref == refid, next_pos, tlen, cig, n_cig, l_seq, smpl);
            for (int i = 0; i < l_seq; ++i) { x->seq16[i] = (sq[i >> 1] >> ((~i & 1) << 2)) & 15; x->qual[i] = ql[i]; }
            if (O.illumina13) for (int i = 0; i < l_seq; ++i) x->qual[i] = x->qual[i] > 31 ? (uint8_t)(x->qual[i] - 31) : 0;
            r->pend = x;
            return;
        }
    }
    for (;;) {
        if (!r->have_line) {
            if (getline(&r->line, &r->line_cap, r->fp) <= 0) { r->done = 1; return; }
        }
        r->have_line = 0;
        char *line = r->line;
        { size_t l = strlen(line); while (l && (line[l - 1] == '\n' || line[l - 1] == '\r')) line[--l] = 0; }
        char *fld[12]; int nf = 0; char *rest = NULL;
        for (char *s = line; nf < 11 && s; ) { fld[nf++] = s; s = strchr(s, '\t'); if (s) *s++ = 0; rest = s; }
        if (nf < 11) continue;
        const int flag = atoi(fld[1]), mapq = atoi(fld[4]), pos = atoi(fld[3]) - 1;
        const int on = !strcmp(fld[2], contig);
        if (on) r->seen_contig = 1;
        if (r->seen_contig && (!on || pos >= reg_end) && !(flag & 4)) { r->done = 1; return; }
        if (!on || !read_passes(flag, mapq)) continue;
        int ncig = 0;
        for (const char *c = fld[5]; *c && *c != '*'; ) {
            char *e; const long l = strtol(c, &e, 10);
            const char *ops = "MIDNSHP=X", *o = *e ? strchr(ops, *e) : NULL;
            if (!o || ncig == 4096) DIE("bad CIGAR in %s\n", r->path);
            cig[ncig++] = (uint32_t)l << 4 | (uint32_t)(o - ops);
            c = e + 1;
        }
        if (!overlaps(pos, ref_span_end(pos, cig, ncig), reg_beg, reg_end)) continue;
        if (!target_keeps_read(contig, pos, ref_span_end(pos, cig, ncig) - 1)) continue;
        const char *rg = NULL;
        for (char *t = rest; t && *t; ) {                                    /* the optional fields: RG:Z:<id> */
            char *e = strchr(t, '\t'); if (e) *e = 0;
            if (!strncmp(t, "RG:Z:", 5)) { rg = t + 5; break; }
            t = e ? e + 1 : NULL;
        }
        const int smpl = sample_of(sf, rg);
        if (smpl < 0) continue;
        const int lq = fld[9][0] == '*' ? 0 : (int)strlen(fld[9]);
        lrec_t *x = lrec_new(fld[0], flag, pos, mapq, !strcmp(fld[6], "=") || !strcmp(fld[6], fld[2]), atoi(fld[7]) - 1, atoi(fld[8]), cig, ncig, lq, smpl);
        const int noq = fld[10][0] == '*' && !fld[10][1];
        for (int i = 0; i < lq; ++i) { x->seq16[i] = (uint8_t)nt16_of(fld[9][i]); x->qual[i] = noq ? 0xff : (uint8_t)(fld[10][i] - 33); }
        if (O.illumina13) for (int i = 0; i < lq; ++i) x->qual[i] = x->qual[i] > 31 ? (uint8_t)(x->qual[i] - 31) : 0;
        r->pend = x;
        return;
    }
}

/* ---- parsing beside the device: up to N_PARSERS threads, thread t owning the readers f = t, t + N, ...  A thread parses the
 * next read of each of its files in turn into that file's ring and sleeps when all its rings are full; the main thread takes the
 * reads from the rings in file order, as it took them from the files.  (Parsing SAM text / inflating BAM was a quarter of a run's
 * wall time and waited for the device and the record writer: profiles/r4_sam_driver_probe.txt.)  One region at a time: the
 * threads are started when the region's files are open and joined before they are closed. ---- */
static int RQ_CAP = 8192;      /* reads a file's ring holds: 8192, fewer with many files (about a million reads waiting in all) */
#define N_PARSERS 8
struct parser {
    pthread_t th; pthread_mutex_t mu; pthread_cond_t data, space;
    reader_t *rdr; const sfile_t *sf; int first, step, n_files; const char *contig; int stop;
};
static void *parser_main(void *arg)
{
    struct parser *p = arg;
    for (;;) {
        int progress = 0, live = 0;
        for (int f = p->first; f < p->n_files; f += p->step) {
            reader_t *r = &p->rdr[f];
            if (r->q_done) continue;
            ++live;
            pthread_mutex_lock(&p->mu);
            const int room = RQ_CAP - r->q_n, stop = p->stop;
            pthread_mutex_unlock(&p->mu);
            if (stop) return NULL;
            if (!room) continue;
            int got = 0; lrec_t *batch[64];
            while (got < 64 && got < room) {                       /* parsed outside the lock, handed over in batches */
                reader_parse(r, p->contig, &p->sf[f]);
                if (!r->pend) break;
                batch[got++] = r->pend; r->pend = NULL;
            }
            pthread_mutex_lock(&p->mu);
            for (int i = 0; i < got; ++i) { r->q[(r->q_rd + r->q_n) % RQ_CAP] = batch[i]; ++r->q_n; }
            if (got < 64 && got < room) r->q_done = 1;              /* the file has nothing more for this region */
            pthread_cond_broadcast(&p->data);
            pthread_mutex_unlock(&p->mu);
            progress += got;
        }
        if (!live) return NULL;
        if (!progress) {                                            /* every ring of this thread is full: wait for the consumer */
            pthread_mutex_lock(&p->mu);
            int full = 1;
            for (int f = p->first; f < p->n_files && full; f += p->step) if (!p->rdr[f].q_done && p->rdr[f].q_n < RQ_CAP) full = 0;
            if (full && !p->stop) pthread_cond_wait(&p->space, &p->mu);
            const int stop = p->stop;
            pthread_mutex_unlock(&p->mu);
            if (stop) return NULL;
        }
    }
}
static struct parser parsers[N_PARSERS]; static int n_parsers;
static void parsers_start(reader_t *rdr, const sfile_t *sf, int F, const char *contig)
{
    n_parsers = F < N_PARSERS ? F : N_PARSERS;
    RQ_CAP = (1 << 20) / (F > 0 ? F : 1); if (RQ_CAP > 8192) RQ_CAP = 8192; if (RQ_CAP < 64) RQ_CAP = 64;
    for (int f = 0; f < F; ++f) { rdr[f].q = grow(NULL, (size_t)RQ_CAP * sizeof *rdr[f].q); rdr[f].q_rd = rdr[f].q_n = rdr[f].q_done = 0; rdr[f].head = NULL; rdr[f].drained = 0; rdr[f].owner = &parsers[f % n_parsers]; }
    for (int t = 0; t < n_parsers; ++t) {
        struct parser *p = &parsers[t];
        memset(p, 0, sizeof *p);
        pthread_mutex_init(&p->mu, NULL); pthread_cond_init(&p->data, NULL); pthread_cond_init(&p->space, NULL);
        p->rdr = rdr; p->sf = sf; p->first = t; p->step = n_parsers; p->n_files = F; p->contig = contig;
        if (pthread_create(&p->th, NULL, parser_main, p)) DIE("cannot start a parsing thread\n");
    }
}
static void parsers_stop(reader_t *rdr, int F)
{
    for (int t = 0; t < n_parsers; ++t) {
        struct parser *p = &parsers[t];
        pthread_mutex_lock(&p->mu); p->stop = 1; pthread_cond_broadcast(&p->space); pthread_mutex_unlock(&p->mu);
        pthread_join(p->th, NULL);
        pthread_mutex_destroy(&p->mu); pthread_cond_destroy(&p->data); pthread_cond_destroy(&p->space);
    }
    for (int f = 0; f < F; ++f) {
        for (int i = 0; i < rdr[f].q_n; ++i) lrec_free(rdr[f].q[(rdr[f].q_rd + i) % RQ_CAP]);
        free(rdr[f].q); rdr[f].q = NULL; rdr[f].q_n = 0;
        lrec_free(rdr[f].head); rdr[f].head = NULL;
    }
    n_parsers = 0;
}
/* the next read of the file into r->head (NULL when the file has no more for the region) */
static void reader_fetch(reader_t *r)
{
    if (r->head || r->drained) return;
    struct parser *p = r->owner;
    pthread_mutex_lock(&p->mu);
    while (!r->q_n && !r->q_done) pthread_cond_wait(&p->data, &p->mu);
    if (r->q_n) { r->head = r->q[r->q_rd]; r->q_rd = (r->q_rd + 1) % RQ_CAP; if (r->q_n-- == RQ_CAP) pthread_cond_signal(&p->space); }
    else r->drained = 1;
    pthread_mutex_unlock(&p->mu);
}

/* the ##contig lines of the VCF header from the first file's dictionary (mpileup.c:533-540) */
static void header_contigs(const reader_t *r, vio_hdr *h)
{
    if (r->is_bam) { for (int i = 0; i < r->n_ref; ++i) contig_line(h, r->ref_name[i], (int)strlen(r->ref_name[i]), r->ref_len[i]); return; }
    for (const char *l = r->text; l && *l; ) {
        if (!strncmp(l, "@SQ\t", 4)) {
            const char *e = strchr(l, '\n'), *sn = strstr(l, "\tSN:"), *ln = strstr(l, "\tLN:");
            if (sn && ln && (!e || (sn < e && ln < e))) { sn += 4; contig_line(h, sn, (int)strcspn(sn, "\t\r\n"), atol(ln + 4)); }
        }
        l = strchr(l, '\n'); if (l) ++l;
    }
}

/* overlap_push (htslib sam.c) over the reads of one sample in file order: which pairs tweak_overlap_quality sees */
static int find_pairs(const pool_t *P, int r0, int r1, int32_t *pa, int32_t *pb)
{
    int np = 0, nb = 1;
    while (nb < 2 * (r1 - r0) + 1) nb <<= 1;
    int32_t *tab = malloc((size_t)nb * sizeof *tab);                         /* open addressing on the read name */
    uint8_t *paired = calloc((size_t)(r1 - r0) + 1, 1);
    for (int i = 0; i < nb; ++i) tab[i] = -1;
    for (int r = r0; r < r1; ++r) {
        const int f = P->flag[r];
        if ((f & 8) || !(f & 2)) continue;
        if (!P->rnext_same[r] || (abs(P->isize[r]) >= 2 * P->lq[r] && P->mpos[r] >= P->end[r])) continue;
        uint32_t h = 2166136261u;
        for (const char *c = P->qname[r]; *c; ++c) h = (h ^ (uint8_t)*c) * 16777619u;
        int slot = (int)(h & (uint32_t)(nb - 1));
        while (tab[slot] >= 0 && strcmp(P->qname[tab[slot]], P->qname[r])) slot = (slot + 1) & (nb - 1);
        if (tab[slot] < 0) {
            if (P->mpos[r] >= P->pos[r] || ((f & 1) && P->mpos[r] == -1)) tab[slot] = r;
        } else if (!paired[tab[slot] - r0]) {
            const int a = tab[slot];
            paired[a - r0] = 1;                    /* the slot stays occupied (probe chains); the name is done */
            if (P->end[a] > P->pos[r]) { pa[np] = a; pb[np] = r; ++np; }
        }
    }
    free(tab); free(paired);
    return np;
}

#define INSCNS_CAP 256

typedef struct { const uint8_t *pl, *sp; const uint16_t *dp4, *adf, *adr, *scr; const int32_t *qs; } planes_t;        /* host copies of bcfgpu_mplp_out's planes */

static void planes_free(planes_t *p) { free((void *)p->pl); free((void *)p->sp); free((void *)p->dp4); free((void *)p->adf); free((void *)p->adr); free((void *)p->scr); free((void *)p->qs); memset(p, 0, sizeof *p); }

static void put_counts(const char *lead, const int32_t *f, const int32_t *r, int n)
{
    fputs(lead, LN);
    for (int j = 0; j < n; ++j) fprintf(LN, "%s%d", j ? "," : "", (f ? f[j] : 0) + (r ? r[j] : 0));
}

/* the samples' columns of a record on their way to the writer: integer arrays, one per FORMAT key; the buffers only grow */
typedef struct { int32_t *col[12]; size_t cap[12]; int width[12], nk; } fmtcols_t;
static inline int32_t *next_col(fmtcols_t *C, int S, int w)                         /* the next key's array: S samples of w numbers */
{
    const int i = C->nk++; const size_t need = (size_t)S * (size_t)w;
    C->width[i] = w;
    if (C->cap[i] < need) { C->cap[i] = need; C->col[i] = grow(C->col[i], need * 4); }
    return C->col[i];
}

/* what bcf_call2bcf writes into a record, in its order (bam2bcf.c:756-906); alleles: the ready REF\tALT text.
 * bytes != NULL: the record's per-sample part, encoded as BCF2 (--device-records, bcfgpu_mplp_encode_bcf) or formatted as VCF text
 * (--device-text, bcfgpu_mplp_encode_vcf) on the device already, is bytes[off[k], off[k + 1]); the planes are not read then */
static void print_record(const char *contig, int pos1, const char *alleles, const char *prefix, const bcfgpu_site *c,
                         const planes_t *pp, size_t k, int S, const uint8_t *bytes, const uint64_t *off)
{
    const uint8_t *indiv = bytes ? bytes + off[k] : NULL; const size_t l_indiv = bytes ? (size_t)(off[k + 1] - off[k]) : 0;
    const int na = c->n_alleles;
    fprintf(LN, "%s\t%d\t.\t%s\t0\t.\t%sDP=%u", contig, pos1, alleles, prefix, c->ori_depth);
    if (O.fmt_flag & BCFGPU_INFO_ADF) put_counts(";ADF=", c->adf_tot, NULL, na);
    if (O.fmt_flag & BCFGPU_INFO_ADR) put_counts(";ADR=", NULL, c->adr_tot, na);
    if (O.fmt_flag & BCFGPU_INFO_AD)  put_counts(";AD=", c->adf_tot, c->adr_tot, na);
    if (O.fmt_flag & BCFGPU_INFO_DPR) put_counts(";DPR=", c->adf_tot, c->adr_tot, na);
    if (O.fmt_flag & BCFGPU_INFO_SCR) fprintf(LN, ";SCR=%d", c->scr_tot);
    fputs(";I16=", LN);
    for (int j = 0; j < 16; ++j) {
        /* %g of a whole number below a million is its digits: most of the sixteen sums are (counts, sums of qualities) */
        const double v = (double)(float)c->anno[j];
        if (j) fputc(',', LN);
        if (v >= 0 && v < 1e6 && v == (double)(long)v && !(v == 0 && signbit(v))) {
            char t[8]; int n = 0; long u = (long)v;
            do { t[n++] = (char)('0' + u % 10); u /= 10; } while (u);
            while (n) fputc(t[--n], LN);
        } else fprintf(LN, "%g", v);
    }
    fputs(";QS=", LN);
    for (int j = 0; j < na; ++j) fprintf(LN, "%s%g", j ? "," : "", (double)c->qsum[j]);
    /* the bias statistics: HUGE_VAL = the tag is left out (bam2bcf.c:835-840) */
    {
        const char *tag[6] = { "VDB", "SGB", "RPB", "MQB", "MQSB", "BQB" };
        const float val[6] = { c->vdb, c->seg_bias, c->mwu_pos, c->mwu_mq, c->mwu_mqs, c->mwu_bq };
        for (int j = 0; j < 6; ++j) if (val[j] != HUGE_VALF) fprintf(LN, ";%s=%g", tag[j], (double)val[j]);
    }
    fprintf(LN, ";MQ0F=%g", c->ori_depth ? (double)((float)c->mq0 / (float)c->ori_depth) : 0.);
    fputs("\tPL", LN);
    if (O.fmt_flag & BCFGPU_FMT_DP) fputs(":DP", LN);
    if (O.fmt_flag & BCFGPU_FMT_DV) fputs(":DV", LN);
    if (O.fmt_flag & BCFGPU_FMT_SP) fputs(":SP", LN);
    if (O.fmt_flag & BCFGPU_FMT_DP4) fputs(":DP4", LN);
    if (O.fmt_flag & BCFGPU_FMT_ADF) fputs(":ADF", LN);
    if (O.fmt_flag & BCFGPU_FMT_ADR) fputs(":ADR", LN);
    if (O.fmt_flag & BCFGPU_FMT_AD) fputs(":AD", LN);
    if (O.fmt_flag & BCFGPU_FMT_DPR) fputs(":DPR", LN);
    if (O.fmt_flag & BCFGPU_FMT_SCR) fputs(":SCR", LN);
    if (O.fmt_flag & BCFGPU_FMT_QS) fputs(":QS", LN);
    if (indiv) {
        end_head();
        if (O.dt_on ? vio_write_record_text(RUN.fout, RUN.hdr, ln_buf, indiv, l_indiv) : vio_write_record_indiv(RUN.fout, RUN.hdr, ln_buf, indiv, l_indiv)) { fprintf(stderr, "%s\n", vio_error()); exit(1); }
        rewind(LN);
        if (O.dt_on) ++RUN.n_dev_text; else ++RUN.n_dev_records;
        return;
    }
    const int x = na * (na + 1) / 2;
    const size_t Ss = (size_t)S;
    /* the samples' columns go to the writer as integer arrays, one per FORMAT key in the order of the keys above (a printf call
     * per number, and a parse of every number on the way into a BCF record, were three fifths of a run's wall time at 40 samples) */
    static fmtcols_t C;
    C.nk = 0;
    { int32_t *a = next_col(&C, S, x); for (int s = 0; s < S; ++s) for (int j = 0; j < x; ++j) a[(size_t)s * x + j] = pp->pl[(k * BCFGPU_MAX_PL + j) * Ss + s]; }
    const uint16_t *d = pp->dp4 + k * 4 * Ss;                                /* FORMAT/DP, DV, DP4 from DP4 (bam2bcf.c:851-886) */
    if (O.fmt_flag & BCFGPU_FMT_DP) { int32_t *a = next_col(&C, S, 1); for (int s = 0; s < S; ++s) a[s] = d[s] + d[Ss + s] + d[2 * Ss + s] + d[3 * Ss + s]; }
    if (O.fmt_flag & BCFGPU_FMT_DV) { int32_t *a = next_col(&C, S, 1); for (int s = 0; s < S; ++s) a[s] = d[2 * Ss + s] + d[3 * Ss + s]; }
    if (O.fmt_flag & BCFGPU_FMT_SP) { int32_t *a = next_col(&C, S, 1); for (int s = 0; s < S; ++s) a[s] = pp->sp[k * Ss + s]; }
    if (O.fmt_flag & BCFGPU_FMT_DP4) { int32_t *a = next_col(&C, S, 4); for (int s = 0; s < S; ++s) for (int j = 0; j < 4; ++j) a[(size_t)s * 4 + j] = d[(size_t)j * Ss + s]; }
    for (int which = 0; which < 4; ++which) {                                /* ADF, ADR, AD, DPR */
        static const int bit[4] = { BCFGPU_FMT_ADF, BCFGPU_FMT_ADR, BCFGPU_FMT_AD, BCFGPU_FMT_DPR };
        if (!(O.fmt_flag & bit[which])) continue;
        int32_t *a = next_col(&C, S, na);
        for (int s = 0; s < S; ++s)
            for (int j = 0; j < na; ++j) {
                const int f = pp->adf[(k * 5 + j) * Ss + s], r = pp->adr[(k * 5 + j) * Ss + s];
                a[(size_t)s * na + j] = which == 0 ? f : which == 1 ? r : f + r;
            }
    }
    if (O.fmt_flag & BCFGPU_FMT_SCR) { int32_t *a = next_col(&C, S, 1); for (int s = 0; s < S; ++s) a[s] = pp->scr[k * Ss + s]; }
    if (O.fmt_flag & BCFGPU_FMT_QS) { int32_t *a = next_col(&C, S, na); for (int s = 0; s < S; ++s) for (int j = 0; j < na; ++j) a[(size_t)s * na + j] = pp->qs[(k * 5 + j) * Ss + s]; }
    end_head();
    if (vio_write_record_int(RUN.fout, RUN.hdr, ln_buf, C.nk, C.width, (const int32_t *const *)C.col)) { fprintf(stderr, "%s\n", vio_error()); exit(1); }
    rewind(LN);
}

/* bcfgpu_mpileup over a tile; the site records and the planes come back to the host.  keep_*: the device copies of the
 * site records / PL / DP4 stay allocated for the caller (--gvcf works on them), else they are freed. */
/* dev != NULL (--device-records, --device-text): only the site records come back; the planes stay in HBM for bcfgpu_mplp_encode_bcf / _vcf (and --gvcf) and
 * are the caller's to free (mplp_out_free) */
static void mplp_out_free(bcfgpu_ctx *ctx, bcfgpu_mplp_out *mo)
{
    bcfgpu_free(ctx, mo->site); bcfgpu_free(ctx, mo->pl); bcfgpu_free(ctx, mo->dp4); bcfgpu_free(ctx, mo->adf); bcfgpu_free(ctx, mo->adr);
    bcfgpu_free(ctx, mo->qs); bcfgpu_free(ctx, mo->scr); bcfgpu_free(ctx, mo->sp);
    memset(mo, 0, sizeof *mo);
}
static void run_mpileup(bcfgpu_ctx *ctx, const bcfgpu_tile *tile, int n, bcfgpu_site **site, planes_t *pp, void **keep_site, void **keep_pl, void **keep_dp4,
                        bcfgpu_mplp_out *dev)
{
    void *d[8]; uint8_t *h[8];
    bcfgpu_mplp_out mo; memset(&mo, 0, sizeof mo);
    for (int w = 0; w < 8; ++w) {
        const size_t nb = bcfgpu_mplp_out_bytes(ctx, n, w);
        CHECK(bcfgpu_malloc(ctx, nb, &d[w]));
        if (w) CHECK(bcfgpu_memset(ctx, d[w], 0, nb));
    }
    mo.site = d[0]; mo.pl = d[1]; mo.dp4 = d[2]; mo.adf = d[3]; mo.adr = d[4]; mo.qs = d[5]; mo.scr = d[6]; mo.sp = d[7];
    CHECK(bcfgpu_mpileup(ctx, tile, &mo));
    CHECK(bcfgpu_sync(ctx));
    if (dev) {
        const size_t nb = bcfgpu_mplp_out_bytes(ctx, n, 0);
        *site = malloc(nb ? nb : 1);
        CHECK(bcfgpu_memcpy_d2h(ctx, *site, d[0], nb));
        CHECK(bcfgpu_sync(ctx));
        memset(pp, 0, sizeof *pp);
        *dev = mo;
        if (keep_site) { *keep_site = d[0]; *keep_pl = d[1]; *keep_dp4 = d[2]; }
        return;
    }
    for (int w = 0; w < 8; ++w) {
        const size_t nb = bcfgpu_mplp_out_bytes(ctx, n, w);
        h[w] = malloc(nb ? nb : 1);
        CHECK(bcfgpu_memcpy_d2h(ctx, h[w], d[w], nb));
    }
    CHECK(bcfgpu_sync(ctx));
    *site = (bcfgpu_site *)h[0];
    pp->pl = h[1]; pp->dp4 = (const uint16_t *)h[2]; pp->adf = (const uint16_t *)h[3]; pp->adr = (const uint16_t *)h[4]; pp->qs = (const int32_t *)h[5];
    pp->scr = (const uint16_t *)h[6]; pp->sp = h[7];
    for (int w = 3; w < 8; ++w) bcfgpu_free(ctx, d[w]);
    if (keep_site) { *keep_site = d[0]; *keep_pl = d[1]; *keep_dp4 = d[2]; }
    else { bcfgpu_free(ctx, d[0]); bcfgpu_free(ctx, d[1]); bcfgpu_free(ctx, d[2]); }
}

/* The per-sample blocks of a tile's records from the planes in HBM: the size pass tells how many bytes, the second call writes them.
 * emit: HOST [n], which sites have a record.  rec / off: HOST, malloc'ed: the blocks back to back, and where each starts. */
typedef struct { bcfgpu_ctx *ctx; int n; const bcfgpu_mplp_out *mo; const uint8_t *d_emit; } enc_arg;
static int encode_blocks(void *arg, void *d_buf, uint64_t cap, uint64_t *d_off, uint64_t *nb)
{
    const enc_arg *a = arg;
    return O.dt_on ? bcfgpu_mplp_encode_vcf(a->ctx, a->n, a->mo, a->d_emit, d_buf, cap, d_off, nb)             /* VCF text for -O v|z */
                 : bcfgpu_mplp_encode_bcf(a->ctx, a->n, a->mo, RUN.dr_key, a->d_emit, d_buf, cap, d_off, nb);    /* BCF2 for -O u|b */
}
static void encode_records(bcfgpu_ctx *ctx, int n, const bcfgpu_mplp_out *mo, const uint8_t *emit, uint8_t **rec, uint64_t **off)
{
    enc_arg a = { ctx, n, mo, dev_upload(ctx, emit, (size_t)n) };
    encode_two_pass(ctx, encode_blocks, &a, O.dt_on ? "bcfgpu_mplp_encode_vcf" : "bcfgpu_mplp_encode_bcf", (size_t)n + 1, rec, off);
    bcfgpu_free(ctx, (void *)a.d_emit);
}

typedef struct { char *contig; int beg, end, open; } region_t;                /* 0-based [beg, end); open: to wherever the reads end (no END given) */
#define OPEN_END 0x3fffffff

/* ---- the device context, re-created when a tile needs more room than the last one had; device: which one (shard_or_device) ---- */
static int device;
static bcfgpu_ctx *ctx; static int ctx_S, ctx_sites; static uint64_t ctx_reads;
static int ctx_fits(int S, int n_sites, uint64_t n_reads) { return ctx && ctx_S == S && n_sites <= ctx_sites && n_reads <= ctx_reads; }
static void ensure_ctx(int S, int n_sites, uint64_t n_reads)
{
    if (ctx_fits(S, n_sites, n_reads)) return;
    uint64_t rng = 0; int have_rng = 0;                                       /* errmod_cal's generator is the process's: it moves to the new context */
    if (ctx) { uint32_t nw = 0; CHECK(bcfgpu_truncated_cells(ctx, &nw)); RUN.n_wide_cells += nw; rng = bcfgpu_errmod_state(ctx); have_rng = 1; bcfgpu_destroy(ctx); ctx = NULL; }
    bcfgpu_cfg cfg; memset(&cfg, 0, sizeof cfg);
    ctx_S = S; ctx_sites = n_sites > ctx_sites ? n_sites : ctx_sites; ctx_reads = n_reads + n_reads / 2 + 4096;
    cfg.device = device; cfg.n_smpl = S; cfg.max_sites = ctx_sites; cfg.max_reads = ctx_reads;   /* every base is in <= 1 column */
    cfg.min_baseQ = O.min_baseQ; cfg.capQ = 60; cfg.errmod_theta = 0.; cfg.fmt_flag = O.fmt_flag;
    cfg.call_theta = 1.1e-3; cfg.n_grp = 1; cfg.ploidy_max = 2;
    CHECK(bcfgpu_create(&cfg, &ctx));
    if (have_rng) CHECK(bcfgpu_errmod_seed(ctx, rng));
}

/* ---- gVCF blocks across tiles (and adjacent regions): the reference's gvcf_write keeps a block open over any distance
 * (gvcf.c:88-226).  bcfgpu_gvcf_blocks ends every block with its call; the block that reaches a tile's last column is held
 * back here and joined with the first block of the next tile when gvcf_write would have gone on: the same sequence, the
 * next position, the same depth range (gvcf.c:130-131).  Per sample the smallest DP and the smallest (PL[1], PL[2]) pair in
 * that order; PL[0], REF and INFO/QS stay the first record's (gvcf.c:160-210). ---- */
static struct { int on, S; char *contig; int start_pos, end1, min_dp, range; char ref; float qs0, qs1; int32_t *dp; uint8_t *pl; } PB;
static void block_line(const char *contig, int start_pos, int end1, int min_dp, char refc, float qs0, float qs1, const uint8_t *pl, const int32_t *dp, int S)
{
    fprintf(LN, "%s\t%d\t.\t%c\t<*>\t.\t.\t", contig, start_pos + 1, refc);
    if (start_pos + 1 < end1) fprintf(LN, "END=%d;", end1);                   /* gvcf.c:150-151 */
    fprintf(LN, "MinDP=%d;QS=%g,%g\tPL:DP", min_dp, (double)qs0, (double)qs1);
    for (int s = 0; s < S; ++s) fprintf(LN, "\t%d,%d,%d:%d", pl[s], pl[(size_t)S + s], pl[2 * (size_t)S + s], dp[s]);
    end_record(RUN.fout, RUN.hdr);
}
static void pending_flush(void)
{
    if (!PB.on) return;
    block_line(PB.contig, PB.start_pos, PB.end1, PB.min_dp, PB.ref, PB.qs0, PB.qs1, PB.pl, PB.dp, PB.S);
    PB.on = 0;
}
static int pending_joins(const char *contig, const bcfgpu_gvcf_block *B) { return PB.on && !strcmp(PB.contig, contig) && B->start_pos == PB.end1 && B->range == PB.range; }
static void pending_merge(const bcfgpu_gvcf_block *B, const uint8_t *pl, const int32_t *dp)
{
    const int S = PB.S;
    PB.end1 = B->end1; if (B->min_dp < PB.min_dp) PB.min_dp = B->min_dp;
    for (int s = 0; s < S; ++s) {
        if (dp[s] < PB.dp[s]) PB.dp[s] = dp[s];
        const uint8_t a = pl[(size_t)S + s], c = pl[2 * (size_t)S + s];
        if (a < PB.pl[(size_t)S + s] || (a == PB.pl[(size_t)S + s] && c < PB.pl[2 * (size_t)S + s])) { PB.pl[(size_t)S + s] = a; PB.pl[2 * (size_t)S + s] = c; }
    }
}
static void pending_set(const char *contig, const bcfgpu_gvcf_block *B, char refc, float qs0, float qs1, const uint8_t *pl, const int32_t *dp, int S)
{
    if (!PB.dp || PB.S != S) { PB.dp = grow(PB.dp, (size_t)S * 4); PB.pl = grow(PB.pl, (size_t)S * 3); PB.S = S; }
    free(PB.contig); PB.contig = strdup(contig);
    PB.on = 1; PB.start_pos = B->start_pos; PB.end1 = B->end1; PB.min_dp = B->min_dp; PB.range = B->range; PB.ref = refc; PB.qs0 = qs0; PB.qs1 = qs1;
    memcpy(PB.dp, dp, (size_t)S * 4); memcpy(PB.pl, pl, (size_t)S * 3);
}

/* ---- a tile's results: what tile_device() computes on the main thread, stage by stage, and emit_tile() writes beside the device
 * stages of the next tile.  Host copies only: sites, planes or encoded bytes, the indel columns' results, the gVCF blocks.
 * tile_device() fills one in place and hands it over by value (emit_submit); from then on it is the record writer's, which frees its
 * arrays (tile_out_free).  The pending gVCF block (PB) and the output are the writer's while it runs: whoever else needs them waits
 * for it (emit_wait).
 *
 * Which column gets a record is decided once per tile, in these arrays, and nowhere else:
 *     visit[k]     column k lies in the targets (target_keeps_column, one call per column per tile)            record_rule_columns
 *     col_live[k]  it has a read and is visited: it gets a SNP record or lies in a gVCF block
 *     ind_col[j]   the column of site j of the indel tile (the j-th candidate where gap_prep returned 0)      indel_candidates
 *     ind_rec[j]   site j has an indel record: bcf_call_combine found an ALT allele there (ret == 0)         mpileup_passes
 *     snp_rec[k]   column k has a SNP record: live and not swallowed by a gVCF block                          record_rule_snps
 * (A candidate column is visited and has a read -- col_indel counts entries of the column -- so an indel record's column is live.)
 * The candidate list, the argument of bcfgpu_errmod_plan_visit, the brk bytes of bcfgpu_gvcf_blocks, the emit masks of the device
 * encoders and the record loop read them.  The encoders write only what snp_rec / ind_rec say and the record loop takes their
 * offsets by site: one rule, so a record cannot get another record's sample columns. ---- */
typedef struct {
    int n_sites, t0, t1, S; const char *contig, *ref;
    int32_t *col_n; uint8_t *col_indel;               /* bcfgpu_pool_pileup: the reads of a column; some read of it is followed by an indel */
    uint8_t *visit, *col_live, *snp_rec, *ind_rec; int32_t *ind_col;          /* the record rule, above */
    int nc, nlive; int32_t *cand, *live;              /* the candidate columns; site j of the indel tile is candidate live[j] */
    int32_t *g_types, *g_maxins, *g_indelreg, *g_support; float *g_frac; int8_t *g_inscns;      /* bcfgpu_gap_prep_tile, per candidate */
    bcfgpu_site *site, *isite; planes_t snp_planes, ind_planes;               /* the two passes of bcfgpu_mpileup */
    int32_t *gv_blk, *gv_dp; bcfgpu_gvcf_block *gv_block; uint8_t *gv_pl;     /* --gvcf: the block of a column or -1; the blocks */
    int open_block;                                   /* the block that reaches the tile's last column and may go on in the next tile, or -1 */
    uint8_t *snp_bytes, *ind_bytes; uint64_t *snp_off, *ind_off;      /* --device-records, --device-text: the records' per-sample blocks instead of the planes */
} tile_out_t;
static void tile_out_free(tile_out_t *R)
{
    free(R->col_n); free(R->col_indel); free(R->visit); free(R->col_live); free(R->snp_rec); free(R->ind_rec); free(R->ind_col); free(R->cand); free(R->live);
    free(R->g_types); free(R->g_maxins); free(R->g_indelreg); free(R->g_support); free(R->g_frac); free(R->g_inscns);
    free(R->site); planes_free(&R->snp_planes); free(R->isite); planes_free(&R->ind_planes);
    free(R->gv_blk); free(R->gv_block); free(R->gv_dp); free(R->gv_pl);
    free(R->snp_bytes); free(R->snp_off); free(R->ind_bytes); free(R->ind_off);
}

static char ref_base(int r) { return "ACGTN"[r < 0 || r > 4 ? 4 : r]; }
/* column k lies inside a gVCF block: one line when the block ends */
static void emit_block_column(const tile_out_t *R, int k)
{
    const int b = R->gv_blk[k], S = R->S;
    const bcfgpu_gvcf_block *B = &R->gv_block[b];
    if (B->first_site == k && PB.on && !pending_joins(R->contig, B)) pending_flush();   /* the block starts: does it continue the one held back? */
    if (B->last_site != k) return;
    const bcfgpu_site *f = &R->site[B->first_site];
    const char refc = ref_base(f->ori_ref);
    const uint8_t *bpl = R->gv_pl + (size_t)b * 3 * S; const int32_t *bdp = R->gv_dp + (size_t)b * S;
    if (PB.on) pending_merge(B, bpl, bdp);                                   /* (a block that did not join was flushed at its first site) */
    else if (b == R->open_block) pending_set(R->contig, B, refc, f->qsum[0], f->qsum[1], bpl, bdp, S);
    else block_line(R->contig, B->start_pos, B->end1, B->min_dp, refc, f->qsum[0], f->qsum[1], bpl, bdp, S);
    if (PB.on && b != R->open_block) pending_flush();                        /* joined, and it ends inside this tile */
}
/* REF <tab> ALT of a SNP record */
static void snp_alleles(const bcfgpu_site *c, char als[64])
{
    int o = 0;
    als[o++] = ref_base(c->ori_ref); als[o++] = '\t';
    for (int j = 1; j < c->n_alleles; ++j) {
        if (j > 1) als[o++] = ',';
        if (j == c->unseen) { memcpy(als + o, "<*>", 3); o += 3; } else als[o++] = ref_base(c->a[j]);
    }
    if (c->n_alleles < 2) als[o++] = '.';
    als[o] = 0;
}
/* REF <tab> ALT of the indel record of site j of the indel tile (bam2bcf.c:767-790), malloc'ed, and its INFO prefix */
static char *indel_alleles(const tile_out_t *R, int j, char prefix[64])
{
    const int i = R->live[j], p = R->t0 + R->ind_col[j], ireg = R->g_indelreg[i], mi = R->g_maxins[i];
    const char *ref = R->ref;
    char *txt = malloc((size_t)(5 * (ireg + mi + 8)) + 64);
    int t = 0;
    for (int q = 0; q <= ireg; ++q) txt[t++] = ref[p + q];
    txt[t++] = '\t';
    for (int a = 1; a < 4 && R->isite[j].a[a] >= 0; ++a) {
        const int ai = R->isite[j].a[a], ty = R->g_types[i * 4 + ai];
        if (a > 1) txt[t++] = ',';
        txt[t++] = ref[p];
        if (ty < 0) { for (int q = p + 1 - ty; q < p + 1 + ireg; ++q) txt[t++] = ref[q]; }
        else {
            for (int q = 0; q < ty; ++q) txt[t++] = ref_base(R->g_inscns[(size_t)i * 4 * INSCNS_CAP + (size_t)ai * mi + q]);
            for (int q = p + 1; q < p + 1 + ireg; ++q) txt[t++] = ref[q];
        }
    }
    txt[t] = 0;
    snprintf(prefix, 64, "INDEL;IDV=%d;IMF=%g;", R->g_support[i], (double)R->g_frac[i]);
    return txt;
}
/* the record loop: the SNP record of a column (or its share of a gVCF block), then its indel record (mpileup.c:343-366) */
static void emit_tile(tile_out_t *R)
{
    const double tw1 = O.want_timing ? now_s() : 0.;
    for (int k = 0, j = 0; k < R->n_sites; ++k) {
        if (!R->col_live[k]) continue;                                       /* no read, or outside the targets: no record (mpileup.c:330-335) */
        if (!R->snp_rec[k]) emit_block_column(R, k);
        else {
            char als[64];
            pending_flush();                                                 /* a record that cannot join ends the block (gvcf.c:107) */
            snp_alleles(&R->site[k], als);
            print_record(R->contig, R->t0 + k + 1, als, "", &R->site[k], &R->snp_planes, (size_t)k, R->S, R->snp_bytes, R->snp_off);
        }
        while (j < R->nlive && R->ind_col[j] < k) ++j;
        if (j < R->nlive && R->ind_col[j] == k && R->ind_rec[j]) {
            char prefix[64], *als = indel_alleles(R, j, prefix);
            pending_flush();
            print_record(R->contig, R->t0 + k + 1, als, prefix, &R->isite[j], &R->ind_planes, (size_t)j, R->S, R->ind_bytes, R->ind_off);
            free(als);
        }
    }
    /* a column without reads ends a block too (a gap in positions, gvcf.c:131): nothing stays open past it */
    if (O.gv_n && PB.on && (R->open_block < 0 || PB.end1 != R->t1)) pending_flush();
    tile_out_free(R);
    if (O.want_timing) RUN.t_emit += now_s() - tw1;
}

static struct { pthread_t th; pthread_mutex_t mu; pthread_cond_t cv; tile_out_t job; int on, have, busy, stop; } EM;
static void *emit_main(void *arg)
{
    (void)arg;
    for (;;) {
        pthread_mutex_lock(&EM.mu);
        while (!EM.have && !EM.stop) pthread_cond_wait(&EM.cv, &EM.mu);
        if (!EM.have) { pthread_mutex_unlock(&EM.mu); return NULL; }
        tile_out_t j = EM.job; EM.have = 0; EM.busy = 1;
        pthread_cond_broadcast(&EM.cv);
        pthread_mutex_unlock(&EM.mu);
        emit_tile(&j);
        pthread_mutex_lock(&EM.mu); EM.busy = 0; pthread_cond_broadcast(&EM.cv); pthread_mutex_unlock(&EM.mu);
    }
}
/* the worker has written everything handed over so far (before anybody else touches the output, the pending block or the reference) */
static void emit_wait(void)
{
    if (!EM.on) return;
    pthread_mutex_lock(&EM.mu);
    while (EM.have || EM.busy) pthread_cond_wait(&EM.cv, &EM.mu);
    pthread_mutex_unlock(&EM.mu);
}
static void emit_submit(const tile_out_t *j)
{
    if (!EM.on) {
        pthread_mutex_init(&EM.mu, NULL); pthread_cond_init(&EM.cv, NULL);
        if (pthread_create(&EM.th, NULL, emit_main, NULL)) DIE("cannot start the record writer\n");
        EM.on = 1;
    }
    pthread_mutex_lock(&EM.mu);
    while (EM.have) pthread_cond_wait(&EM.cv, &EM.mu);          /* (one tile waiting while one is written) */
    EM.job = *j; EM.have = 1;
    pthread_cond_broadcast(&EM.cv);
    pthread_mutex_unlock(&EM.mu);
}
static void emit_finish(void)
{
    if (!EM.on) return;
    emit_wait();
    pthread_mutex_lock(&EM.mu); EM.stop = 1; pthread_cond_broadcast(&EM.cv); pthread_mutex_unlock(&EM.mu);
    pthread_join(EM.th, NULL);
    EM.on = 0; EM.stop = 0;
}

/* ---- one tile: columns [t0, t1) of `contig` from the reads in P (all the reads that overlap the tile, file-major; file f =
 * [first[f], first[f+1])).  Its host preparation (tile_prepare: the mates' pairs, the per-sample position order) is apart from
 * its device stages (tile_device), so that with --prefetch the next tile is prepared and its pool is on its way to the device
 * while this tile's stages run; the records of the tiles are written in position order either way. ---- */
typedef struct {
    pool_t P;
    int32_t *pa, *pb; int np;                       /* the overlapping mates */
    int S, t0, t1, ref_len; const char *contig, *ref;
} tilejob_t;
static void pool_reads(const pool_t *P, bcfgpu_reads *rd)
{
    memset(rd, 0, sizeof *rd);
    rd->n_reads = P->n; rd->r_pos = P->pos; rd->r_lq = P->lq; rd->r_flag = P->flag; rd->r_ncig = P->ncig; rd->r_cig_off = P->cig_off;
    rd->r_seq_off = P->seq_off; rd->cig = P->cig; rd->seq16 = P->seq16; rd->qual = P->qual; rd->zq = P->zq; rd->r_has_zq = P->has_zq;
}
/* a[r] = a[ord[r]] over n elements of es bytes; scratch: n * es bytes */
static void permute(void *a, size_t es, const int32_t *ord, int n, void *scratch)
{
    for (int r = 0; r < n; ++r) memcpy((char *)scratch + (size_t)r * es, (const char *)a + (size_t)ord[r] * es, es);
    memcpy(a, scratch, (size_t)n * es);
}
static void tile_prepare(tilejob_t *T, const int *first, int F)
{
    pool_t *P = &T->P;
    const int S = T->S;
    const double tw0 = O.want_timing ? now_s() : 0.;
    /* mate overlaps: htslib pairs the reads inside one file's iterator (bam_mplp_init_overlaps, mpileup.c:640) */
    int32_t *pa = malloc((size_t)(P->n + 1) * sizeof *pa), *pb = malloc((size_t)(P->n + 1) * sizeof *pb);
    int np = 0;
    if (!O.no_overlaps) for (int f = 0; f < F; ++f) np += find_pairs(P, first[f], first[f + 1], pa + np, pb + np);
    RUN.tot_pairs += (unsigned long long)np;
    /* a sample fed by several files (mpileup.c:275-293 appends file after file): its reads merged by position, files in
     * order at equal positions, as bcfgpu_pileup wants them; the pairs follow their reads */
    {
        int sorted = 1;
        int32_t *last = malloc((size_t)S * sizeof *last);
        for (int s = 0; s < S; ++s) last[s] = INT32_MIN;
        for (int r = 0; r < P->n && sorted; ++r) { if (P->pos[r] < last[P->smpl[r]]) sorted = 0; last[P->smpl[r]] = P->pos[r]; }
        free(last);
        if (!sorted) {
            int32_t *ord = malloc((size_t)P->n * sizeof *ord), *tmp = malloc((size_t)P->n * sizeof *tmp), *inv = malloc((size_t)P->n * sizeof *inv);
            for (int r = 0; r < P->n; ++r) ord[r] = r;
            for (int w = 1; w < P->n; w *= 2) {                              /* bottom-up merge sort: stable */
                for (int lo = 0; lo < P->n; lo += 2 * w) {
                    const int mid = lo + w < P->n ? lo + w : P->n, hi = lo + 2 * w < P->n ? lo + 2 * w : P->n;
                    int i = lo, j = mid, k = lo;
                    while (i < mid && j < hi) tmp[k++] = P->pos[ord[j]] < P->pos[ord[i]] ? ord[j++] : ord[i++];
                    while (i < mid) tmp[k++] = ord[i++];
                    while (j < hi) tmp[k++] = ord[j++];
                }
                int32_t *t = ord; ord = tmp; tmp = t;
            }
            for (int r = 0; r < P->n; ++r) inv[ord[r]] = r;
            void *scratch = malloc((size_t)P->n * sizeof *P->qname);         /* (the widest element) */
            int32_t *i32[12] = { P->pos, P->lq, P->flag, P->ncig, P->cig_off, P->seq_off, P->smpl, P->file, P->end, P->mpos, P->isize, P->rnext_same };
            for (int a = 0; a < 12; ++a) permute(i32[a], 4, ord, P->n, scratch);
            permute(P->mapq, 1, ord, P->n, scratch); permute(P->has_zq, 1, ord, P->n, scratch); permute(P->qname, sizeof *P->qname, ord, P->n, scratch);
            free(scratch);
            for (int i = 0; i < np; ++i) { pa[i] = inv[pa[i]]; pb[i] = inv[pb[i]]; }
            free(ord); free(tmp); free(inv);
        }
    }
    T->pa = pa; T->pb = pb; T->np = np;
    if (O.want_timing) RUN.t_dev += now_s() - tw0;
}

/* ---- the device stages of a prepared tile, each a function over the tile's results R (tile_out_t) and over D, what of the tile
 * stays on the device from one stage to the next ---- */
typedef struct {
    bcfgpu_reads rd;                                  /* the host pool, as the library takes it */
    bcfgpu_tile tile, ti;                             /* the pileup of the tile; the indel tile gap_prep leaves */
    void *d_site, *d_pl, *d_dp4;                      /* --gvcf: the SNP pass's site records, PL and DP4, for bcfgpu_gvcf_blocks */
    bcfgpu_mplp_out snp_dev, ind_dev;                 /* --device-records, --device-text: the planes of both passes, for the encoders */
} tile_dev_t;

/* The pool goes up once (unless it is the context's already: adopted) and stays in HBM: BAQ (new qualities and ZQ bytes for the reads
 * it applies to; not with -B), the mate-overlap tweak, the pileup of the tile -- each on the copy the stage before left there */
static void tile_pileup(tilejob_t *T, int adopted, tile_dev_t *D, tile_out_t *R)
{
    pool_t *P = &T->P;
    pool_reads(P, &D->rd);
    if (!adopted) {
        ensure_ctx(R->S, R->n_sites, (uint64_t)P->nbase + 64);
        CHECK(bcfgpu_pool_upload(ctx, &D->rd, NULL, P->mapq));
    }
    if (O.baq_flag) CHECK(bcfgpu_pool_baq(ctx, T->ref, T->ref_len, O.baq_flag, NULL));
    CHECK(bcfgpu_pool_overlap_tweak(ctx, T->np, T->pa, T->pb));
    free(T->pa); free(T->pb); T->pa = T->pb = NULL;
    R->col_n = malloc((size_t)(R->n_sites + 1) * sizeof *R->col_n);
    R->col_indel = malloc((size_t)R->n_sites + 1);
    CHECK(bcfgpu_pool_pileup(ctx, P->smpl, NULL, R->t0, R->t1, T->ref, T->ref_len, &D->tile, R->col_n, R->col_indel));
    RUN.tot_entries += (unsigned long long)D->tile.n_reads;
}
/* a column outside the targets is passed over before bcf_call_glfgen (mpileup.c:330-335), one without a read gives no record */
static void record_rule_columns(tile_out_t *R)
{
    R->visit = malloc((size_t)R->n_sites + 1); R->col_live = malloc((size_t)R->n_sites + 1);
    for (int k = 0; k < R->n_sites; ++k) {
        R->visit[k] = (uint8_t)target_keeps_column(R->contig, R->t0 + k);
        R->col_live[k] = R->visit[k] && R->col_n[k] != 0;
    }
}
/* Indel candidates (mpileup.c:354-365): candidate columns -> bcf_call_gap_prep.  Everything stays in HBM: the entries of the
 * candidates that pass the pooled support filter, the stage on the pool bcfgpu_pileup left there, p->aux straight into the indel
 * pass's tile D->ti -- the candidates where it returned 0, in order (the host pool is passed for its ZQ bytes) */
static void indel_candidates(tile_dev_t *D, tile_out_t *R)
{
    const int S = R->S;
    R->cand = malloc((size_t)(R->n_sites + 1) * sizeof *R->cand);
    for (int k = 0; k < R->n_sites; ++k)
        if (!O.no_indels && R->col_indel[k] && R->col_n[k] < O.max_indel_depth * S && R->visit[k]) R->cand[R->nc++] = k;      /* mpileup.c:354 */
    const int nc = R->nc;
    if (nc) {
        bcfgpu_indel_in in; memset(&in, 0, sizeof in);
        in.n_sites = nc; in.n_smpl = S; in.ref = R->ref;
        in.openQ = O.openQ; in.extQ = O.extQ; in.tandemQ = O.tandemQ; in.min_support = O.min_support; in.per_sample_flt = O.per_sample_flt; in.min_frac = O.min_frac;
        bcfgpu_indel_out out; memset(&out, 0, sizeof out);
        int32_t *gret = malloc((size_t)nc * 4);
        R->g_types = malloc((size_t)nc * 16); R->g_inscns = malloc((size_t)nc * 4 * INSCNS_CAP); R->g_maxins = malloc((size_t)nc * 4);
        R->g_indelreg = malloc((size_t)nc * 4); R->g_support = malloc((size_t)nc * 4); R->g_frac = malloc((size_t)nc * 4);
        out.ret = gret; out.p_aux = NULL; out.indel_types = R->g_types; out.inscns = R->g_inscns; out.maxins = R->g_maxins;
        out.indelreg = R->g_indelreg; out.max_support = R->g_support; out.max_frac = R->g_frac;
        /* (with BAQ the ZQ bytes are the pool's, in HBM; with -B the reads' own tags, if any, go up from the host) */
        CHECK(bcfgpu_gap_prep_tile(ctx, nc, R->cand, O.baq_flag ? NULL : &D->rd, &in, &out, INSCNS_CAP, &D->ti));
        R->live = malloc((size_t)nc * 4);
        for (int i = 0; i < nc; ++i) if (gret[i] == 0) R->live[R->nlive++] = i;
        free(gret);
    }
    R->ind_col = malloc((size_t)(R->nlive + 1) * 4);                          /* the SNP-tile column of every site of the indel tile */
    for (int j = 0; j < R->nlive; ++j) R->ind_col[j] = R->cand[R->live[j]];
}
/* Before either pass of bcf_call_glfgen runs: errmod_cal's draw for cells of more than 255 reads is planned over BOTH passes of the
 * tile in the reference's visit order -- position by position the SNP pass, then the indel pass where gap_prep returned >= 0
 * (bcfgpu_errmod_plan); errmod_cal spends no draw on a column that is not visited */
static void errmod_plan(tile_dev_t *D, const tile_out_t *R)
{
    CHECK(bcfgpu_errmod_plan_visit(ctx, &D->tile, R->visit, R->nlive ? &D->ti : NULL, R->ind_col, NULL));
}
/* the SNP pass, then the indel pass on the tile gap_prep left (the columns where it returned 0, mpileup.c:354-360) */
static void mpileup_passes(tile_dev_t *D, tile_out_t *R)
{
    run_mpileup(ctx, &D->tile, R->n_sites, &R->site, &R->snp_planes, O.gv_n ? &D->d_site : NULL, &D->d_pl, &D->d_dp4, DEV_ON ? &D->snp_dev : NULL);
    if (R->nlive) run_mpileup(ctx, &D->ti, R->nlive, &R->isite, &R->ind_planes, NULL, NULL, NULL, DEV_ON ? &D->ind_dev : NULL);
    R->ind_rec = malloc((size_t)R->nlive + 1);
    for (int j = 0; j < R->nlive; ++j) R->ind_rec[j] = R->isite[j].ret == 0 && R->col_live[R->ind_col[j]];
}
/* --gvcf: reference-only records collapse into blocks (gvcf_write, gvcf.c:88-226) on the planes still in HBM */
static void gvcf_tile(tile_dev_t *D, tile_out_t *R)
{
    const int n_sites = R->n_sites, S = R->S;
    int32_t *pos = malloc((size_t)n_sites * 4), nb = 0; uint8_t *brk = calloc((size_t)n_sites, 1);
    for (int k = 0; k < n_sites; ++k) { pos[k] = R->t0 + k; if (!R->col_live[k]) brk[k] |= 2; }
    for (int j = 0; j < R->nlive; ++j) if (R->ind_rec[j]) brk[R->ind_col[j]] |= 1;           /* an indel record follows the SNP record */
    void *d_pos, *d_brk, *d_blk, *d_min, *d_block, *d_gdp, *d_gpl;
    CHECK(bcfgpu_malloc(ctx, (size_t)n_sites * 4, &d_pos)); CHECK(bcfgpu_malloc(ctx, (size_t)n_sites, &d_brk));
    CHECK(bcfgpu_malloc(ctx, (size_t)n_sites * 4, &d_blk)); CHECK(bcfgpu_malloc(ctx, (size_t)n_sites * 4, &d_min));
    CHECK(bcfgpu_malloc(ctx, (size_t)n_sites * sizeof(bcfgpu_gvcf_block), &d_block));
    CHECK(bcfgpu_malloc(ctx, (size_t)n_sites * S * 4, &d_gdp)); CHECK(bcfgpu_malloc(ctx, (size_t)n_sites * 3 * S, &d_gpl));
    CHECK(bcfgpu_memcpy_h2d(ctx, d_pos, pos, (size_t)n_sites * 4)); CHECK(bcfgpu_memcpy_h2d(ctx, d_brk, brk, (size_t)n_sites));
    bcfgpu_gvcf_in gi; memset(&gi, 0, sizeof gi);
    gi.n_sites = n_sites; gi.n_range = O.gv_n; gi.dp_range = O.gv_range; gi.pos = d_pos; gi.brk = d_brk;
    gi.site = D->d_site; gi.pl = D->d_pl; gi.dp4 = D->d_dp4;
    bcfgpu_gvcf_out go = { d_blk, d_min, d_block, d_gdp, d_gpl };
    CHECK(bcfgpu_gvcf_blocks(ctx, &gi, &go, &nb));
    R->gv_blk = malloc((size_t)n_sites * 4); R->gv_block = malloc((size_t)(nb + 1) * sizeof *R->gv_block);
    R->gv_dp = malloc((size_t)(nb + 1) * S * 4); R->gv_pl = malloc((size_t)(nb + 1) * 3 * S);
    CHECK(bcfgpu_memcpy_d2h(ctx, R->gv_blk, d_blk, (size_t)n_sites * 4)); CHECK(bcfgpu_memcpy_d2h(ctx, R->gv_block, d_block, (size_t)nb * sizeof *R->gv_block));
    CHECK(bcfgpu_memcpy_d2h(ctx, R->gv_dp, d_gdp, (size_t)nb * S * 4)); CHECK(bcfgpu_memcpy_d2h(ctx, R->gv_pl, d_gpl, (size_t)nb * 3 * S));
    CHECK(bcfgpu_sync(ctx));
    /* open at the tile's end: the last column is in a block and no indel record follows it */
    if (R->gv_blk[n_sites - 1] >= 0 && !(brk[n_sites - 1] & 1)) R->open_block = R->gv_blk[n_sites - 1];
    bcfgpu_free(ctx, d_pos); bcfgpu_free(ctx, d_brk); bcfgpu_free(ctx, d_blk); bcfgpu_free(ctx, d_min); bcfgpu_free(ctx, d_block);
    bcfgpu_free(ctx, d_gdp); bcfgpu_free(ctx, d_gpl); free(pos); free(brk);
    if (!DEV_ON) { bcfgpu_free(ctx, D->d_site); bcfgpu_free(ctx, D->d_pl); bcfgpu_free(ctx, D->d_dp4); }      /* (else: freed with the other planes, encode_tile) */
}
/* a live column has a SNP record unless a gVCF block swallowed it */
static void record_rule_snps(tile_out_t *R)
{
    R->snp_rec = malloc((size_t)R->n_sites + 1);
    for (int k = 0; k < R->n_sites; ++k) R->snp_rec[k] = R->col_live[k] && !(R->gv_blk && R->gv_blk[k] >= 0);
}
/* --device-records, --device-text: the per-sample blocks of the sites that have a record come to the host as BCF2 bytes or as VCF text */
static void encode_tile(tile_dev_t *D, tile_out_t *R)
{
    encode_records(ctx, R->n_sites, &D->snp_dev, R->snp_rec, &R->snp_bytes, &R->snp_off);
    if (R->nlive) encode_records(ctx, R->nlive, &D->ind_dev, R->ind_rec, &R->ind_bytes, &R->ind_off);
    mplp_out_free(ctx, &D->snp_dev);
    if (R->nlive) mplp_out_free(ctx, &D->ind_dev);
}
/* adopted: the tile's pool is the context's already (bcfgpu_pool_adopt).  The records go to the writer (emit_tile), which runs
 * beside the next tile's device stages */
static void tile_device(tilejob_t *T, int adopted)
{
    const double tw0 = O.want_timing ? now_s() : 0.;
    tile_dev_t D; memset(&D, 0, sizeof D);
    tile_out_t R; memset(&R, 0, sizeof R);
    R.n_sites = T->t1 - T->t0; R.t0 = T->t0; R.t1 = T->t1; R.S = T->S; R.contig = T->contig; R.ref = T->ref; R.open_block = -1;
    tile_pileup(T, adopted, &D, &R);
    record_rule_columns(&R);
    indel_candidates(&D, &R);
    errmod_plan(&D, &R);
    mpileup_passes(&D, &R);
    if (O.gv_n) gvcf_tile(&D, &R);
    record_rule_snps(&R);
    if (DEV_ON) encode_tile(&D, &R);
    if (O.want_timing) RUN.t_dev += now_s() - tw0;
    emit_submit(&R);
}

/* ---- the tile loop's two orders.  Without --prefetch a tile is prepared, uploaded and run before the next one is read.  With
 * it the pools alternate between two page-locked sets of buffers: tile i + 1 is read and prepared, its pool staged
 * (bcfgpu_pool_stage returns with the copies queued), then tile i, whose pool the context holds, runs its device stages under
 * those copies, and bcfgpu_pool_adopt makes the staged pool the context's.  Tile i's host arrays live until its stages are done
 * (bcfgpu_pool_pileup reads the sample of each read, -B's bcfgpu_gap_prep_tile the ZQ tags).  The -C side context, the depth
 * cap and the files are ahead by one tile; the draws of errmod_cal, the gVCF block and the records keep the tiles' order. ---- */
static tilejob_t TJ[2]; static int tj_fill; static tilejob_t *tj_run;          /* tj_run: staged and adopted, its device stages still to run */
static void tile_drain(void) { if (tj_run) { tile_device(tj_run, 1); tj_run = NULL; } }
static void tile_submit(tilejob_t *T, const int *first, int F)
{
    tile_prepare(T, first, F);
    if (!O.prefetch) { tile_device(T, 0); return; }
    const int n_sites = T->t1 - T->t0;
    /* a tile that needs a larger context: the one before runs first, on the context that holds its pool */
    if (!ctx_fits(T->S, n_sites, (uint64_t)T->P.nbase + 64)) { tile_drain(); ensure_ctx(T->S, n_sites, (uint64_t)T->P.nbase + 64); }
    bcfgpu_reads rd;
    pool_reads(&T->P, &rd);
    CHECK(bcfgpu_pool_stage(ctx, &rd, NULL, T->P.mapq));
    tile_drain();
    const double ta0 = O.want_timing ? now_s() : 0.;
    CHECK(bcfgpu_pool_adopt(ctx));
    if (O.want_timing) RUN.t_adopt += now_s() - ta0;
    tj_run = T; tj_fill ^= 1;
}

/* ---- the live window: the reads of every file that passed the filters and the depth cap and may still cover a column ---- */
typedef struct { lrec_t **r; int n, cap; } lwin_t;
static void lwin_push(lwin_t *w, lrec_t *x) { if (w->n == w->cap) { w->cap = w->cap ? 2 * w->cap : 256; w->r = grow(w->r, (size_t)w->cap * sizeof *w->r); } w->r[w->n++] = x; }

static void pool_clear(pool_t *P) { P->n = 0; P->ncigs = 0; P->nbase = 0; }
static void pool_add_rec(pool_t *P, int file, const lrec_t *x)
{
    pool_add(P, file, x->smpl, x->qname, x->flag, x->pos, x->mapq, x->rnext_same, x->mpos, x->isize, x->cig, x->ncig, x->lq, x->seq16, x->qual);
}

/* mpileup -C INT (mpileup.c:234-241) for a batch of reads: after BAQ, sam_cap_mapq lowers the mapping quality of reads with
 * many mismatches or drops them; then the -q and orphan filters, which read_passes() left for here.  keep[i] = 0: dropped. */
static bcfgpu_ctx *cap_ctx;
static void cap_batch(lrec_t **b, int n, int S, const char *ref, int ref_len, uint8_t *keep)
{
    static pool_t Q;
    pool_clear(&Q);
    for (int i = 0; i < n; ++i) pool_add_rec(&Q, 0, b[i]);
    if (!cap_ctx) {
        bcfgpu_cfg c0; memset(&c0, 0, sizeof c0);
        c0.device = device; c0.n_smpl = S; c0.max_sites = 1; c0.max_reads = 64; c0.min_baseQ = O.min_baseQ; c0.capQ = 60; c0.n_grp = 1; c0.ploidy_max = 2;
        CHECK(bcfgpu_create(&c0, &cap_ctx));
    }
    bcfgpu_reads r0;
    pool_reads(&Q, &r0);
    /* the batch goes up once; BAQ and the cap run on that copy (the qualities sam_cap_mapq sees are BAQ's) */
    CHECK(bcfgpu_pool_upload(cap_ctx, &r0, NULL, Q.mapq));
    if (O.baq_flag) CHECK(bcfgpu_pool_baq(cap_ctx, ref, ref_len, O.baq_flag, NULL));
    int32_t *capv = malloc((size_t)(n + 1) * sizeof *capv);
    CHECK(bcfgpu_pool_cap_mapq(cap_ctx, ref, ref_len, O.cap_thres, capv));
    for (int i = 0; i < n; ++i) {
        keep[i] = capv[i] >= 0;
        if (keep[i] && b[i]->mapq > capv[i]) b[i]->mapq = capv[i];
        if (b[i]->mapq < O.min_mq) keep[i] = 0;
        if (!O.keep_orphans && (b[i]->flag & 1) && !(b[i]->flag & 2)) keep[i] = 0;
    }
    free(capv);
}
/* mpileup -d: the iterator's depth cap of file f over a batch of its reads, which bcfgpu_depth_cap_push wants as arrays.  keep[i] = 0: dropped */
static void depth_cap_batch(bcfgpu_depth_state *dcap, lrec_t **b, int n, int f, uint8_t *keep)
{
    int32_t *pos = malloc((size_t)n * 4), *ncg = malloc((size_t)n * 4), *coff = malloc((size_t)n * 4), *fl = malloc((size_t)n * 4);
    size_t nc = 0; for (int i = 0; i < n; ++i) nc += (size_t)b[i]->ncig;
    uint32_t *cg = malloc((nc + 1) * 4);
    nc = 0;
    for (int i = 0; i < n; ++i) { pos[i] = b[i]->pos; ncg[i] = b[i]->ncig; coff[i] = (int32_t)nc; fl[i] = f; memcpy(cg + nc, b[i]->cig, (size_t)b[i]->ncig * 4); nc += (size_t)b[i]->ncig; }
    bcfgpu_reads r0; memset(&r0, 0, sizeof r0);
    r0.n_reads = n; r0.r_pos = pos; r0.r_ncig = ncg; r0.r_cig_off = coff; r0.cig = cg;
    CHECK(bcfgpu_depth_cap_push(dcap, &r0, fl, keep));
    free(pos); free(ncg); free(coff); free(fl); free(cg);
}

static region_t parse_region(const char *s)
{
    region_t g; memset(&g, 0, sizeof g);
    const char *colon = strrchr(s, ':');
    g.beg = 0; g.end = -1;
    if (!colon) { g.contig = strdup(s); return g; }
    g.contig = strndup(s, (size_t)(colon - s));
    char *e; long b = strtol(colon + 1, &e, 10);
    if (e == colon + 1) { free(g.contig); g.contig = strdup(s); return g; }          /* a colon inside the contig's name */
    g.beg = (int)(b > 0 ? b - 1 : 0);
    if (*e == '-' && e[1]) g.end = (int)strtol(e + 1, NULL, 10);
    else if (*e != '-') g.end = (int)b;                                              /* "chr:pos": one position */
    return g;
}

/* ---- --gpus N: the parent of the shard processes.  It touches no device: it starts one process per shard, each writing its
 * record stream (uncompressed BCF) to an anonymous temporary file the parent holds open, and writes the streams out in shard
 * order -- which is genomic order -- once the shards are through.  With --gvcf the last block of a shard and the first of the
 * next are joined where gvcf_write would have gone on (the same rule as between two tiles).
 * (The records of `mpileup` are every column's PL / DP planes, encoded on the host of the shard that computed them: a device
 * gather -- bcfgpu_gather_bytes, what the call-side drivers use for their compacted call records -- would carry host-made
 * bytes through HBM and back.) ---- */
typedef struct { char *line; int is_block, pos1, end1, min_dp; } gline_t;
static int gline_parse(gline_t *g, char *line)
{
    g->line = line; g->is_block = 0;
    char *f[10]; int nf = 0;
    char *dup = strdup(line);
    for (char *s = dup; nf < 10 && s; ) { f[nf++] = s; s = strchr(s, '\t'); if (s) *s++ = 0; }
    if (nf >= 9 && !strcmp(f[4], "<*>") && strstr(f[7], "MinDP=") && !strcmp(f[8], "PL:DP")) {
        g->is_block = 1; g->pos1 = atoi(f[1]);
        const char *e = strstr(f[7], "END="); g->end1 = e == f[7] || (e && e[-1] == ';') ? atoi(e + 4) : g->pos1;
        g->min_dp = atoi(strstr(f[7], "MinDP=") + 6);
    }
    free(dup);
    return g->is_block;
}
static int dp_range_of(int min_dp) { int r = 0; while (r < O.gv_n && min_dp >= O.gv_range[r]) ++r; return r; }
/* a (held back) + b, both block lines of the same contig: the joined line, malloc'ed */
static char *gline_join(const gline_t *a, const gline_t *b)
{
    char *fa[10] = {0}, *fb[10] = {0}; int na = 0, nb = 0;
    char *da = strdup(a->line), *db = strdup(b->line);
    for (char *s = da; na < 9 && s; ) { fa[na++] = s; s = strchr(s, '\t'); if (s) *s++ = 0; if (na == 9) fa[9] = s; }
    for (char *s = db; nb < 9 && s; ) { fb[nb++] = s; s = strchr(s, '\t'); if (s) *s++ = 0; if (nb == 9) fb[9] = s; }
    const char *qs = strstr(fa[7], "QS=");
    char *out = NULL; size_t len = 0;
    FILE *m = open_memstream(&out, &len);
    fprintf(m, "%s\t%d\t.\t%s\t<*>\t.\t.\tEND=%d;MinDP=%d;%s\tPL:DP", fa[0], a->pos1, fa[3], b->end1, a->min_dp < b->min_dp ? a->min_dp : b->min_dp, qs ? qs : "");
    char *sa = fa[9], *sb = fb[9];
    while (sa && sb && *sa && *sb) {
        int pa[3], pb_[3], da_, db_;
        if (sscanf(sa, "%d,%d,%d:%d", &pa[0], &pa[1], &pa[2], &da_) != 4 || sscanf(sb, "%d,%d,%d:%d", &pb_[0], &pb_[1], &pb_[2], &db_) != 4) DIE("--gvcf: cannot join two blocks\n");
        if (pb_[1] < pa[1] || (pb_[1] == pa[1] && pb_[2] < pa[2])) { pa[1] = pb_[1]; pa[2] = pb_[2]; }
        fprintf(m, "\t%d,%d,%d:%d", pa[0], pa[1], pa[2], da_ < db_ ? da_ : db_);
        sa = strchr(sa, '\t'); if (sa) ++sa;
        sb = strchr(sb, '\t'); if (sb) ++sb;
    }
    fclose(m); free(da); free(db);
    return out;
}

static const char *shard_transport = "";
static int run_shards(int n_gpus, int argc0, char **argv0, int first_file, const region_t *reg, int n_reg)
{
    /* the shards: the columns of all regions, in order, cut into n_gpus contiguous runs */
    long total = 0;
    for (int i = 0; i < n_reg; ++i) total += reg[i].end - reg[i].beg;
    const int n_sh = (long)n_gpus < total ? n_gpus : (total > 0 ? (int)total : 1);
    pid_t *pid = malloc((size_t)n_sh * sizeof *pid);
    int *rfd = malloc((size_t)n_sh * sizeof *rfd);
    extern char **environ;
    for (int k = 0; k < n_sh; ++k) {
        const long c0 = total * k / n_sh, c1 = total * (k + 1) / n_sh;
        char *rl = NULL; size_t rlen = 0; FILE *m = open_memstream(&rl, &rlen);
        long at = 0; int nr = 0;
        for (int i = 0; i < n_reg; ++i) {
            const long lo = at > c0 ? at : c0, hi = at + (reg[i].end - reg[i].beg) < c1 ? at + (reg[i].end - reg[i].beg) : c1;
            if (lo < hi) {
                if (reg[i].open && hi == at + (reg[i].end - reg[i].beg)) fprintf(m, "%s%s:%ld-", nr++ ? "," : "", reg[i].contig, reg[i].beg + (lo - at) + 1);
                else fprintf(m, "%s%s:%ld-%ld", nr++ ? "," : "", reg[i].contig, reg[i].beg + (lo - at) + 1, reg[i].beg + (hi - at));
            }
            at += reg[i].end - reg[i].beg;
        }
        fclose(m);
        /* the shard's records go to shared memory: an anonymous memory file (memfd_create: pages in RAM, no name in any file
         * system, nothing anyone could predict or replace) that this process holds open; the shard inherits the descriptor and
         * opens it by number.  (Where the kernel has no memfd_create: an unlinked temporary file, held the same way.) */
        int tfd = (int)syscall(SYS_memfd_create, "bcfgpu_shard", 0u);
        if (tfd >= 0) shard_transport = "memfd (shared memory)";
        else {
            FILE *tf = tmpfile();
            if (!tf) DIE("tmpfile failed\n");
            tfd = dup(fileno(tf));
            fclose(tf);
            shard_transport = "unlinked temporary file";
        }
        if (tfd < 0 || fcntl(tfd, F_SETFD, 0)) DIE("shard descriptor\n");
        char **av = malloc((size_t)(argc0 + 16) * sizeof *av);
        int n = 0;
        char sk[24], sfd[40]; snprintf(sk, sizeof sk, "%d", k); snprintf(sfd, sizeof sfd, "/dev/fd/%d", tfd);
        av[n++] = argv0[0]; av[n++] = "--shard"; av[n++] = strdup(sk);
        for (int i = 1; i < first_file; ++i) {                   /* the options, without -O / -o FILE / --output / --gpus / -r / -f and the old positional region */
            const char *o = argv0[i];
            if (!strcmp(o, "--gpus") || !strcmp(o, "--output") || !strcmp(o, "-O") || !strcmp(o, "-r") || !strcmp(o, "--regions") || !strcmp(o, "-R") || !strcmp(o, "--regions-file") || !strcmp(o, "-f") || !strcmp(o, "--fasta-ref")) { ++i; continue; }
            if (!strncmp(o, "-O", 2) && o[2]) continue;
            if (!strcmp(o, "-o")) { char *e; strtol(argv0[i + 1], &e, 10); if (*e) { ++i; continue; } }
            if (o[0] != '-') break;                              /* the positional form: ref.fa contig beg end come from -f / -r below */
            av[n++] = argv0[i];
            if (o[0] == '-' && i + 1 < first_file && argv0[i + 1][0] != '-' && strcmp(o, "-B") && strcmp(o, "-E") && strcmp(o, "-A") && strcmp(o, "-p") && strcmp(o, "-I") && strcmp(o, "-6") && strcmp(o, "--illumina1.3+") && strcmp(o, "--timing") && strcmp(o, "--prefetch") && strcmp(o, "--device-records") && strcmp(o, "--device-text") && strcmp(o, "-x") && strcmp(o, "--ignore-overlaps") && strcmp(o, "--no-version")
                && strcmp(o, "--ignore-RG") && strcmp(o, "--list-samples")) av[n++] = argv0[++i];
        }
        av[n++] = "-f"; av[n++] = (char *)O.ref_path; av[n++] = "-r"; av[n++] = rl;
        av[n++] = "-O"; av[n++] = "u"; av[n++] = "--output"; av[n++] = strdup(sfd);
        for (int i = first_file; i < argc0; ++i) av[n++] = argv0[i];
        av[n] = NULL;
        if (posix_spawn(&pid[k], "/proc/self/exe", NULL, NULL, av, environ)) {
            for (int j = 0; j < k; ++j) { kill(pid[j], SIGTERM); waitpid(pid[j], NULL, 0); }          /* no orphans behind a failed start */
            DIE("cannot start shard %d\n", k);
        }
        rfd[k] = tfd;
        free(av);
    }
    int bad = 0;
    for (int k = 0; k < n_sh; ++k) { int st = 0; if (waitpid(pid[k], &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st)) bad = 1; }
    if (bad) DIE("a shard failed\n");
    fprintf(stderr, "[bcfgpu_sam] %d region shards, one process each; their record streams (uncompressed BCF through %s) are emitted in shard order on the host\n", n_sh, shard_transport);
    char *lb = NULL; size_t lcap = 0;
    gline_t held; char *held_line = NULL; memset(&held, 0, sizeof held);
    for (int k = 0; k < n_sh; ++k) {
        char path[40]; snprintf(path, sizeof path, "/dev/fd/%d", rfd[k]);
        vio_file *fk = vio_open_read(path);
        vio_hdr *hk = fk ? vio_read_hdr(fk) : NULL;
        if (!fk || !hk) DIE("shard %d: %s\n", k, vio_error());
        if (k == 0) {
            RUN.hdr = hk;
            RUN.fout = vio_open_write(O.out_path, O.out_mode);
            if (!RUN.fout || vio_write_hdr(RUN.fout, RUN.hdr)) DIE("%s\n", vio_error());
        }
        int rr, first = 1;
        while ((rr = vio_read_line(fk, hk, &lb, &lcap)) > 0) {
            if (!lb[0]) continue;
            gline_t g;
            if (O.gv_n && gline_parse(&g, lb)) {
                /* the shard's first line continues the block the shard before ended with? */
                if (held_line && first && !strncmp(held_line, lb, strcspn(lb, "\t") + 1) && g.pos1 == held.end1 + 1 && dp_range_of(g.min_dp) == dp_range_of(held.min_dp)) {
                    char *j = gline_join(&held, &g);
                    free(held_line); held_line = j; gline_parse(&held, held_line);
                } else {
                    if (held_line) { if (vio_write_line(RUN.fout, RUN.hdr, held_line)) DIE("%s\n", vio_error()); free(held_line); }
                    held_line = strdup(lb); gline_parse(&held, held_line);
                }
            } else {
                if (held_line) { if (vio_write_line(RUN.fout, RUN.hdr, held_line)) DIE("%s\n", vio_error()); free(held_line); held_line = NULL; }
                if (vio_write_line(RUN.fout, RUN.hdr, lb)) DIE("%s\n", vio_error());
            }
            first = 0;
        }
        if (rr < 0) DIE("shard %d: %s\n", k, vio_error());
        vio_close(fk);
        if (k) vio_hdr_free(hk);
    }
    if (held_line) { if (vio_write_line(RUN.fout, RUN.hdr, held_line)) DIE("%s\n", vio_error()); free(held_line); }
    free(lb);
    if (vio_close(RUN.fout)) DIE("%s\n", vio_error());
    return 0;
}

/* ---- the command line ---- */
static void usage(void)
{
    fprintf(stderr, "usage: bcfgpu_sam [-a TAG,..] [--gvcf INT,..] [-O v|z|u|b] [-o out] [-d INT] [-s LIST | -S FILE] [-G FILE] [--ignore-RG]\n"
                    "                  [-B | -E] [-6] [-x] [-A] [-q INT] [-Q INT] [-C INT] [--ff INT] [--rf INT] [-I] [-o INT] [-e INT] [-h INT] [-m INT] [-F FLOAT] [-p] [-L INT]\n"
                    "                  [--tile COLUMNS] [--gpus N] [--prefetch] [--device-records] [--device-text]\n"
                    "                  -f ref.fa [-r CHR[:BEG[-END]],... | -R FILE] [-b FILE] file.sam|file.bam [...]      (as `bcftools mpileup`)\n"
                    "              or  ref.fa contig beg end file.sam|file.bam [...]                    (beg, end 1-based inclusive)\n");
    exit(2);
}
/* mpileup -a (parse_format_flag, mpileup.c:794-826): the names without regard to case, FORMAT tags with or without "FORMAT/" or "FMT/" */
static void annotate_option(const char *arg)
{
    static const struct { const char *name; int bit; } tags[] = {
        { "DP", BCFGPU_FMT_DP }, { "DV", BCFGPU_FMT_DV }, { "SP", BCFGPU_FMT_SP }, { "DP4", BCFGPU_FMT_DP4 }, { "DPR", BCFGPU_FMT_DPR },
        { "AD", BCFGPU_FMT_AD }, { "ADF", BCFGPU_FMT_ADF }, { "ADR", BCFGPU_FMT_ADR }, { "SCR", BCFGPU_FMT_SCR }, { "QS", BCFGPU_FMT_QS },
        { "INFO/DPR", BCFGPU_INFO_DPR }, { "INFO/AD", BCFGPU_INFO_AD }, { "INFO/ADF", BCFGPU_INFO_ADF }, { "INFO/ADR", BCFGPU_INFO_ADR },
        { "INFO/SCR", BCFGPU_INFO_SCR } };
    char *list = strdup(arg);
    for (char *t = strtok(list, ","); t; t = strtok(NULL, ",")) {
        const char *name = !strncasecmp(t, "FORMAT/", 7) ? t + 7 : !strncasecmp(t, "FMT/", 4) ? t + 4 : t;
        size_t i;
        for (i = 0; i < sizeof tags / sizeof tags[0]; ++i)
            if (!strcasecmp(name, tags[i].name) && (name == t || strncasecmp(tags[i].name, "INFO/", 5))) { O.fmt_flag |= tags[i].bit; break; }
        if (i == sizeof tags / sizeof tags[0]) { fprintf(stderr, "Could not parse tag \"%s\" in \"%s\"\n", t, arg); exit(1); }
    }
    free(list);
}
/* The options that only set something are rows of opt_row: name, kind, where it goes.  Kinds: 'f' a flag, the int becomes val;
 * 'i' an int (atoi); 'x' an int in any base (strtol); 'd' a double; 's' a string; '0' and '1' read and not used, without and
 * with an argument.  Every kind but 'f' and '0' takes the next argument. */
static const struct { const char *name; char kind; size_t at; int val; } opt_row[] = {
    { "-f", 's', offsetof(opt_t, ref_path), 0 }, { "--fasta-ref", 's', offsetof(opt_t, ref_path), 0 },              /* mpileup.c:1008,1056 */
    { "-r", 's', offsetof(opt_t, reg_arg), 0 }, { "--regions", 's', offsetof(opt_t, reg_arg), 0 },                  /* mpileup.c:1011,1057 */
    { "-R", 's', offsetof(opt_t, reg_file), 0 }, { "--regions-file", 's', offsetof(opt_t, reg_file), 0 },           /* mpileup.c:1031 */
    { "-b", 's', offsetof(opt_t, file_list), 0 }, { "--bam-list", 's', offsetof(opt_t, file_list), 0 },             /* mpileup.c:1072 */
    { "--output", 's', offsetof(opt_t, out_path), 0 },
    { "-x", 'f', offsetof(opt_t, no_overlaps), 1 }, { "--ignore-overlaps", 'f', offsetof(opt_t, no_overlaps), 1 },  /* mpileup.c:1005 */
    { "-6", 'f', offsetof(opt_t, illumina13), 1 }, { "--illumina1.3+", 'f', offsetof(opt_t, illumina13), 1 },       /* mpileup.c:1057 */
    { "-P", '1', 0, 0 }, { "--platforms", '1', 0, 0 },          /* read and never used by the reference either (mpileup.c:353, 1052) */
    { "--no-version", '0', 0, 0 },                              /* (no ##bcftoolsVersion / ##bcftoolsCommand lines are written anyway) */
    { "--threads", '1', 0, 0 },                                 /* (the output's compression threads: nothing to do here) */
    { "--timing", 'f', offsetof(opt_t, want_timing), 1 }, { "--prefetch", 'f', offsetof(opt_t, prefetch), 1 },
    { "--device-records", 'f', offsetof(opt_t, device_records), 1 }, { "--device-text", 'f', offsetof(opt_t, device_text), 1 },
    { "--ignore-RG", 'f', offsetof(opt_t, ignore_rg), 1 }, { "--list-samples", 'f', offsetof(opt_t, list_only), 1 },
    { "--gpus", 'i', offsetof(opt_t, n_gpus), 0 }, { "--shard", 'i', offsetof(opt_t, shard), 0 },
    { "-d", 'i', offsetof(opt_t, max_depth), 0 },
    { "-B", 'f', offsetof(opt_t, baq_flag), 0 }, { "-E", 'f', offsetof(opt_t, baq_flag), 7 },                       /* mpileup.c:1045,1062 */
    { "-A", 'f', offsetof(opt_t, keep_orphans), 1 }, { "-q", 'i', offsetof(opt_t, min_mq), 0 }, { "-Q", 'i', offsetof(opt_t, min_baseQ), 0 },
    { "-C", 'i', offsetof(opt_t, cap_thres), 0 },                                                                   /* mpileup.c:1069 */
    { "-e", 'i', offsetof(opt_t, extQ), 0 }, { "-h", 'i', offsetof(opt_t, tandemQ), 0 }, { "-m", 'i', offsetof(opt_t, min_support), 0 },
    { "-F", 'd', offsetof(opt_t, min_frac), 0 }, { "-L", 'i', offsetof(opt_t, max_indel_depth), 0 },
    { "-p", 'f', offsetof(opt_t, per_sample_flt), 1 }, { "-I", 'f', offsetof(opt_t, no_indels), 1 },
    { "--ff", 'x', offsetof(opt_t, rflag_filter), 0 }, { "--rf", 'x', offsetof(opt_t, rflag_require), 0 } };
/* 1 and the row applied, or 0: not a row.  *used: the arguments it took, the option's name included */
static int table_option(const char *name, const char *arg, int *used)
{
    for (size_t i = 0; i < sizeof opt_row / sizeof opt_row[0]; ++i) {
        if (strcmp(name, opt_row[i].name)) continue;
        void *at = (char *)&O + opt_row[i].at;
        const char k = opt_row[i].kind;
        *used = k == 'f' || k == '0' ? 1 : 2;
        if (k == 'f') *(int *)at = opt_row[i].val;
        else if (k == 'i') *(int *)at = atoi(arg);
        else if (k == 'x') *(int *)at = (int)strtol(arg, NULL, 0);
        else if (k == 'd') *(double *)at = atof(arg);
        else if (k == 's') *(const char **)at = arg;
        return 1;
    }
    return 0;
}
/* Fills O.  On return argv[1 .. argc) are the input files named on the command line, in both spellings of what to run on:
 * mpileup's own (-f REF [-r CHR[:BEG[-END]],...] files), or "ref.fa contig beg end files".  An option is read while an argument
 * follows it (argc > 2): a trailing option is taken for a file. */
static void parse_options(int *argc_io, char ***argv_io)
{
    int argc = *argc_io; char **argv = *argv_io;
    {   /* mpileup's long option names (mpileup.c:952-1003) are read as their short forms */
        static const char *alias[][2] = {
            { "--count-orphans", "-A" }, { "--no-BAQ", "-B" }, { "--adjust-MQ", "-C" }, { "--max-depth", "-d" }, { "--redo-BAQ", "-E" },
            { "--read-groups", "-G" }, { "--min-MQ", "-q" }, { "--min-BQ", "-Q" }, { "--incl-flags", "--rf" }, { "--excl-flags", "--ff" },
            { "--annotate", "-a" }, { "--output-type", "-O" }, { "--samples", "-s" }, { "--samples-file", "-S" }, { "--ext-prob", "-e" },
            { "--gap-frac", "-F" }, { "--tandem-qual", "-h" }, { "--skip-indels", "-I" }, { "--max-idepth", "-L" }, { "--min-ireads", "-m" },
            { "--open-prob", "-o" }, { "--per-sample-mF", "-p" } };
        for (int i = 1; i < argc; ++i)
            for (size_t k = 0; k < sizeof alias / sizeof alias[0]; ++k) if (!strcmp(argv[i], alias[k][0])) argv[i] = (char *)alias[k][1];
    }
    memset(&O, 0, sizeof O);                                                  /* the defaults: mpileup.c:937-950 */
    O.rflag_filter = 4 | 256 | 512 | 1024; O.target_incl = 1; O.fmt_flag = BCFGPU_INFO_VDB | BCFGPU_INFO_RPB;
    O.max_depth = 250; O.baq_flag = 3; O.min_baseQ = 13; O.max_indel_depth = 250;
    O.openQ = 40; O.extQ = 20; O.tandemQ = 100; O.min_support = 1; O.min_frac = 0.002;
    O.out_mode = 'v'; O.out_path = "-"; O.tile_cols = 16384; O.n_gpus = 1; O.shard = -1;
    while (argc > 2 && argv[1][0] == '-' && argv[1][1]) {
        const char *o = argv[1], *arg = argv[2];
        int used = 2;
        if (table_option(o, arg, &used)) ;
        else if (!strcmp(o, "-a")) annotate_option(arg);
        else if (!strcmp(o, "--gvcf") || !strcmp(o, "-g")) {                  /* (lenient: what atoi makes of every item) */
            char *list = strdup(arg);
            for (char *t = strtok(list, ","); t; t = strtok(NULL, ",")) { if (O.gv_n == 16) DIE("--gvcf: at most 16 limits\n"); O.gv_range[O.gv_n++] = atoi(t); }
            free(list);
            O.fmt_flag |= BCFGPU_FMT_DP;                                      /* mpileup.c:1101-1105 */
        }
        else if (!strcmp(o, "-O")) O.out_mode = arg[0];
        else if (!strncmp(o, "-O", 2) && o[2]) { O.out_mode = o[2]; used = 1; }
        else if (!strcmp(o, "-o")) {                                          /* -o INT: --open-prob, -o FILE: --output (the reference's own rule, mpileup.c:1073-1079) */
            char *e; const long v = strtol(arg, &e, 10);
            if (*e == 0) O.openQ = (int)v; else O.out_path = arg;
        }
        else if (!strcmp(o, "-t") || !strcmp(o, "--targets") || !strcmp(o, "-T") || !strcmp(o, "--targets-file")) {   /* mpileup.c:1033-1051 */
            if (arg[0] == '^') { ++arg; O.target_incl = 0; }
            if (!strcmp(o, "-T") || !strcmp(o, "--targets-file")) target_file(arg);
            else {
                char *list = strdup(arg);
                for (char *t = strtok(list, ","); t; t = strtok(NULL, ",")) target_spec(t);
                free(list);
            }
        }
        else if (!strcmp(o, "-s")) add_samples(arg, 0);                       /* mpileup.c:1058-1059,1087,1016 */
        else if (!strcmp(o, "-S")) add_samples(arg, 1);
        else if (!strcmp(o, "-G")) add_readgroups(arg);
        else if (!strcmp(o, "--tile")) { O.tile_cols = atoi(arg); if (O.tile_cols < 1) DIE("--tile: at least one column\n"); }
        else break;
        argv += used; argc -= used;
    }
    if (O.ref_path) { if (argc < 2 && !O.file_list) usage(); }
    else {
        if (argc < 6) usage();
        O.ref_path = argv[1]; O.pos_region[0] = argv[2]; O.pos_region[1] = argv[3]; O.pos_region[2] = argv[4];
        argv += 4; argc -= 4;
    }
    O.dr_on = O.device_records && (O.out_mode == 'u' || O.out_mode == 'b');   /* BCF output only (text is formatted from the planes on the host) */
    O.dt_on = O.device_text && (O.out_mode == 'v' || O.out_mode == 'z');      /* text output only (BCF has --device-records) */
    O.defer_mq_filters = O.cap_thres > 10;
    *argc_io = argc; *argv_io = argv;
}

/* ---- the run, stage by stage: what main() hands from one stage to the next ---- */
typedef struct {
    int argc0; char **argv0;                          /* the command line as it came (the shards get its options) */
    int n_in, n_pos; char **in_path;                  /* input_files: all of them; those named on the command line (the others: -b) */
    region_t *reg; int n_reg;                         /* regions */
    int F, S; reader_t *rdr; sfile_t *sfile; const char **kept_path;          /* open_inputs: the files kept, their readers and sample maps; output samples */
    char *ref, *ref_name; int ref_len;                /* the contig's sequence (one at a time in memory) */
    bcfgpu_depth_state *dcap; lwin_t *win;            /* per file: the iterator's buffer (mpileup -d); the live window */
    int *first, max_span;                             /* where a file's reads start in the tile's pool; the longest reference span of a read so far */
    long long *n_in_smpl; int *nf_smpl, *lastf_smpl;  /* --list-samples: reads entering the pileup and files, per sample */
} job_t;

/* The lines of a list file as -b (input paths, read_file_list, mpileup.c:733-790) and -R (regions) read them: line by line, trailing
 * blanks cut, empty lines passed over; skip_hash (-R): a '#' in the first column starts a comment.  (-S / -G go through read_list:
 * hts_readlist cuts at line ends only and keeps blanks, which next_field then skips.) */
static char **file_lines(const char *path, int skip_hash, int *n)
{
    FILE *f = fopen(path, "r");
    if (!f) DIE("cannot open %s\n", path);
    char **rows = NULL, *ln = NULL; size_t lcap = 0;
    *n = 0;
    while (getline(&ln, &lcap, f) > 0) {
        size_t l = strlen(ln);
        while (l && isspace((unsigned char)ln[l - 1])) ln[--l] = 0;
        if (!l || (skip_hash && ln[0] == '#')) continue;
        rows = grow(rows, (size_t)(*n + 1) * sizeof *rows); rows[(*n)++] = strdup(ln);
    }
    free(ln); fclose(f);
    return rows;
}
/* the input files: those on the command line, then those of -b FILE */
static void input_files(job_t *J, int argc, char **argv)
{
    J->n_in = J->n_pos = argc - 1; J->in_path = argv + 1;
    if (!O.file_list) return;
    int n; char **rows = file_lines(O.file_list, 0, &n);
    if (!n) DIE("No files read from %s\n", O.file_list);
    char **all = grow(NULL, (size_t)(J->n_in + n) * sizeof *all);
    memcpy(all, J->in_path, (size_t)J->n_in * sizeof *all); memcpy(all + J->n_in, rows, (size_t)n * sizeof *all);
    free(rows);
    J->in_path = all; J->n_in += n;
}
static void add_region(job_t *J, region_t g) { J->reg = grow(J->reg, (size_t)(J->n_reg + 1) * sizeof *J->reg); J->reg[J->n_reg++] = g; }
/* the regions: CONTIG BEG END of the five-argument spelling, or -r and -R; neither: open_inputs takes every sequence of the first file */
static void regions(job_t *J)
{
    if (O.pos_region[0]) {
        region_t g; memset(&g, 0, sizeof g);
        g.contig = strdup(O.pos_region[0]); g.beg = atoi(O.pos_region[1]) - 1; g.end = atoi(O.pos_region[2]);      /* 1-based inclusive -> 0-based [beg, end) */
        add_region(J, g);
        return;
    }
    if (O.reg_arg) {
        char *list = strdup(O.reg_arg);
        for (char *t = strtok(list, ","); t; t = strtok(NULL, ",")) add_region(J, parse_region(t));
        free(list);
    }
    if (O.reg_file) {
        /* -R FILE: tab-delimited CHROM, POS and, optionally, END (1-based, inclusive), or CHROM alone */
        int n; char **rows = file_lines(O.reg_file, 1, &n);
        for (int i = 0; i < n; ++i) {
            char *ln = rows[i], *c1 = strchr(ln, '\t'), *c2 = c1 ? strchr(c1 + 1, '\t') : NULL, spec[1200];
            if (!c1) snprintf(spec, sizeof spec, "%s", ln);
            else { *c1 = 0; if (c2) *c2 = 0; snprintf(spec, sizeof spec, "%.1000s:%ld-%ld", ln, atol(c1 + 1), c2 ? atol(c2 + 1) : atol(c1 + 1)); }
            add_region(J, parse_region(spec));
            free(ln);
        }
        free(rows);
        if (!J->n_reg) DIE("no region in %s\n", O.reg_file);
    }
}
/* the sequence names of a file's dictionary: BAM's own, or the @SQ lines of the header text */
static void all_contigs(job_t *J, const reader_t *r)
{
    region_t g; memset(&g, 0, sizeof g); g.end = -1;
    if (r->is_bam) { for (int k = 0; k < r->n_ref; ++k) { g.contig = strdup(r->ref_name[k]); add_region(J, g); } return; }
    for (const char *l = r->text; l && *l; ) {
        if (!strncmp(l, "@SQ\t", 4)) {
            const char *sn = strstr(l, "\tSN:"), *e = strchr(l, '\n');
            if (sn && (!e || sn < e)) { sn += 4; g.contig = strndup(sn, strcspn(sn, "\t\r\n")); add_region(J, g); }
        }
        l = strchr(l, '\n'); if (l) ++l;
    }
}
/* the input files' headers decide the samples (bam_smpl_add_bam) and give the ##contig lines; without -r the first file's
 * dictionary gives the regions */
static void open_inputs(job_t *J)
{
    J->rdr = calloc((size_t)J->n_in, sizeof *J->rdr);
    J->sfile = calloc((size_t)J->n_in, sizeof *J->sfile);
    J->kept_path = calloc((size_t)J->n_in, sizeof *J->kept_path);
    RUN.hdr = vio_hdr_new();
    { char b[4096]; snprintf(b, sizeof b, "##reference=file://%s", O.ref_path); vio_hdr_append(RUN.hdr, b); }
    const int default_regions = !J->n_reg;
    for (int i = 0; i < J->n_in; ++i) {                                       /* F: files kept (mpileup.c:442-455 drops the others) */
        reader_t *r = &J->rdr[J->F];
        reader_open(r, J->in_path[i]);
        if (i == 0 && default_regions) all_contigs(J, r);
        const int keep = add_file(&J->sfile[J->F], J->in_path[i], r->text);
        if (keep && J->F == 0) header_contigs(r, RUN.hdr);
        reader_close(r);
        if (keep) J->kept_path[J->F++] = J->in_path[i];
    }
    if (!J->n_reg) DIE("no region to run on: no -r and no sequence dictionary in the first file\n");
    J->S = SM.nsmpl;
    if (!J->F || !J->S) DIE("no sample left to call\n");
    /* A region without an END runs to wherever the reads end -- past the contig's last base if they do, as the reference's iterator
     * does (reference base N there) */
    for (int i = 0; i < J->n_reg; ++i) if (J->reg[i].end < 0) { J->reg[i].open = 1; J->reg[i].end = OPEN_END; }
}
/* --gpus N: this process becomes the parent of the shards and is through when they are (1); --shard K: which device */
static int shard_or_device(job_t *J)
{
    if (O.list_only) return 0;
    const int n_gpus = O.n_gpus;
    if (n_gpus > 1 && O.shard < 0) {
        /* for the shards an open region is cut at the contig's length and the last piece stays open */
        for (int i = 0; i < J->n_reg; ++i) if (J->reg[i].open) { int len = 0; char *sq = read_contig(O.ref_path, J->reg[i].contig, &len); J->reg[i].end = len > J->reg[i].beg ? len : J->reg[i].beg + 1; free(sq); }
        run_shards(n_gpus, J->argc0, J->argv0, J->argc0 - J->n_pos, J->reg, J->n_reg);
        return 1;
    }
    if (O.shard > 0) { const int nd = bcfgpu_device_count(); device = nd > 0 ? O.shard % nd : 0; if (nd > 1) fprintf(stderr, "[bcfgpu_sam] shard %d on device %d of %d\n", O.shard, device, nd); }
    return 0;
}
static void hdr_line_if(int cond, const char *text) { if (cond) vio_hdr_append(RUN.hdr, text); }
/* the VCF header, in mpileup's order (mpileup.c:510-602); the output is opened and gets it */
static void write_header(const job_t *J)
{
    const int f = O.fmt_flag;
    hdr_line_if(1, "##ALT=<ID=*,Description=\"Represents allele(s) other than observed.\">");
    hdr_line_if(1, "##INFO=<ID=INDEL,Number=0,Type=Flag,Description=\"Indicates that the variant is an INDEL.\">");
    hdr_line_if(1, "##INFO=<ID=IDV,Number=1,Type=Integer,Description=\"Maximum number of raw reads supporting an indel\">");
    hdr_line_if(1, "##INFO=<ID=IMF,Number=1,Type=Float,Description=\"Maximum fraction of raw reads supporting an indel\">");
    hdr_line_if(1, "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Raw read depth\">");
    hdr_line_if(f & BCFGPU_INFO_VDB, "##INFO=<ID=VDB,Number=1,Type=Float,Description=\"Variant Distance Bias for filtering splice-site artefacts in RNA-seq data (bigger is better)\",Version=\"3\">");
    hdr_line_if(f & BCFGPU_INFO_RPB, "##INFO=<ID=RPB,Number=1,Type=Float,Description=\"Mann-Whitney U test of Read Position Bias (bigger is better)\">");
    hdr_line_if(1, "##INFO=<ID=MQB,Number=1,Type=Float,Description=\"Mann-Whitney U test of Mapping Quality Bias (bigger is better)\">");
    hdr_line_if(1, "##INFO=<ID=BQB,Number=1,Type=Float,Description=\"Mann-Whitney U test of Base Quality Bias (bigger is better)\">");
    hdr_line_if(1, "##INFO=<ID=MQSB,Number=1,Type=Float,Description=\"Mann-Whitney U test of Mapping Quality vs Strand Bias (bigger is better)\">");
    hdr_line_if(1, "##INFO=<ID=SGB,Number=1,Type=Float,Description=\"Segregation based metric.\">");
    hdr_line_if(1, "##INFO=<ID=MQ0F,Number=1,Type=Float,Description=\"Fraction of MQ0 reads (smaller is better)\">");
    hdr_line_if(1, "##INFO=<ID=I16,Number=16,Type=Float,Description=\"Auxiliary tag used for calling, see description of bcf_callret1_t in bam2bcf.h\">");
    hdr_line_if(1, "##INFO=<ID=QS,Number=R,Type=Float,Description=\"Auxiliary tag used for calling\">");
    hdr_line_if(1, "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"List of Phred-scaled genotype likelihoods\">");
    hdr_line_if(f & BCFGPU_FMT_DP, "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Number of high-quality bases\">");
    hdr_line_if(f & BCFGPU_FMT_DV, "##FORMAT=<ID=DV,Number=1,Type=Integer,Description=\"Number of high-quality non-reference bases\">");
    hdr_line_if(f & BCFGPU_FMT_DPR, "##FORMAT=<ID=DPR,Number=R,Type=Integer,Description=\"Number of high-quality bases observed for each allele\">");
    hdr_line_if(f & BCFGPU_INFO_DPR, "##INFO=<ID=DPR,Number=R,Type=Integer,Description=\"Number of high-quality bases observed for each allele\">");
    hdr_line_if(f & BCFGPU_FMT_DP4, "##FORMAT=<ID=DP4,Number=4,Type=Integer,Description=\"Number of high-quality ref-fwd, ref-reverse, alt-fwd and alt-reverse bases\">");
    hdr_line_if(f & BCFGPU_FMT_SP, "##FORMAT=<ID=SP,Number=1,Type=Integer,Description=\"Phred-scaled strand bias P-value\">");
    hdr_line_if(f & BCFGPU_FMT_AD, "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Allelic depths (high-quality bases)\">");
    hdr_line_if(f & BCFGPU_FMT_ADF, "##FORMAT=<ID=ADF,Number=R,Type=Integer,Description=\"Allelic depths on the forward strand (high-quality bases)\">");
    hdr_line_if(f & BCFGPU_FMT_ADR, "##FORMAT=<ID=ADR,Number=R,Type=Integer,Description=\"Allelic depths on the reverse strand (high-quality bases)\">");
    hdr_line_if(f & BCFGPU_FMT_QS, "##FORMAT=<ID=QS,Number=R,Type=Integer,Description=\"Phred-score allele quality sum used by `call -mG` and `+trio-dnm`\">");
    hdr_line_if(f & BCFGPU_INFO_AD, "##INFO=<ID=AD,Number=R,Type=Integer,Description=\"Total allelic depths (high-quality bases)\">");
    hdr_line_if(f & BCFGPU_INFO_ADF, "##INFO=<ID=ADF,Number=R,Type=Integer,Description=\"Total allelic depths on the forward strand (high-quality bases)\">");
    hdr_line_if(f & BCFGPU_INFO_SCR, "##INFO=<ID=SCR,Number=1,Type=Integer,Description=\"Number of soft-clipped reads (at high-quality bases)\">");
    hdr_line_if(f & BCFGPU_FMT_SCR, "##FORMAT=<ID=SCR,Number=1,Type=Integer,Description=\"Per-sample number of soft-clipped reads (at high-quality bases)\">");
    hdr_line_if(f & BCFGPU_INFO_ADR, "##INFO=<ID=ADR,Number=R,Type=Integer,Description=\"Total allelic depths on the reverse strand (high-quality bases)\">");
    hdr_line_if(O.gv_n, "##INFO=<ID=END,Number=1,Type=Integer,Description=\"End position of the variant described in this record\">");   /* gvcf.c:42-43 */
    hdr_line_if(O.gv_n, "##INFO=<ID=MinDP,Number=1,Type=Integer,Description=\"Minimum per-sample depth in this gVCF block\">");
    for (int s = 0; s < J->S; ++s) vio_hdr_add_sample(RUN.hdr, SM.smpl[s]);
    if (O.list_only) return;
    RUN.fout = vio_open_write(O.out_path, O.out_mode);
    if (!RUN.fout || vio_write_hdr(RUN.fout, RUN.hdr)) DIE("%s\n", vio_error());
    open_record_stream();
    if (O.dr_on) {
        static const char *key[BCFGPU_BCF_NKEYS] = { "PL", "DP", "DV", "SP", "DP4", "ADF", "ADR", "AD", "DPR", "SCR", "QS" };
        for (int i = 0; i < BCFGPU_BCF_NKEYS; ++i) { RUN.dr_key[i] = vio_hdr_fmt_id(RUN.hdr, key[i]); if (RUN.dr_key[i] < 0) RUN.dr_key[i] = 0; }     /* (a key the flags do not select is not read) */
    }
}

/* ---- the regions, one after the other (mpileup.c:652-683), each streamed through in tiles of O.tile_cols columns: the files are
 * read in step with the tiles (a sorted file no further than the tile's end), a read stays in memory while it can still cover a
 * column, and what is on the device at any time is one tile.  SURVEY 8e: "shards further cut into tiles". ---- */
static void tile_loop_init(job_t *J)
{
    const int F = J->F, S = J->S;
    J->dcap = bcfgpu_depth_cap_new(F, O.max_depth);
    if (!J->dcap) DIE("%s\n", bcfgpu_last_error());
    J->win = calloc((size_t)F, sizeof *J->win);
    TJ[0].P.pinned = TJ[1].P.pinned = O.prefetch && !O.list_only;
    J->first = malloc((size_t)(F + 1) * sizeof *J->first);
    J->n_in_smpl = calloc((size_t)S, sizeof *J->n_in_smpl); J->nf_smpl = calloc((size_t)S, sizeof *J->nf_smpl); J->lastf_smpl = malloc((size_t)S * sizeof *J->lastf_smpl);
    for (int s = 0; s < S; ++s) J->lastf_smpl[s] = -1;
}
/* the reads of file f that start before `limit` come off its ring, through -C (BAQ + sam_cap_mapq + the deferred filters) and the
 * depth cap, into the file's live window */
static void read_file_batch(job_t *J, int f, int limit)
{
    lrec_t **b = NULL; int nb = 0, bcap = 0;
    for (;;) {
        reader_fetch(&J->rdr[f]);
        lrec_t *x = J->rdr[f].head;
        if (!x || x->pos >= limit) break;
        J->rdr[f].head = NULL;
        if (x->end - x->pos > J->max_span) J->max_span = x->end - x->pos;
        if (nb == bcap) { bcap = bcap ? 2 * bcap : 256; b = grow(b, (size_t)bcap * sizeof *b); }
        b[nb++] = x;
    }
    if (!nb) { free(b); return; }
    uint8_t *keep = malloc((size_t)nb);
    memset(keep, 1, (size_t)nb);
    if (O.defer_mq_filters && !O.list_only) cap_batch(b, nb, J->S, J->ref, J->ref_len, keep);
    int m = 0;
    for (int i = 0; i < nb; ++i) { if (keep[i]) b[m++] = b[i]; else lrec_free(b[i]); }
    if (O.max_depth > 0 && m) depth_cap_batch(J->dcap, b, m, f, keep); else memset(keep, 1, (size_t)nb);
    for (int i = 0; i < m; ++i) {
        if (!keep[i]) { lrec_free(b[i]); continue; }
        lwin_push(&J->win[f], b[i]);
        const int s = b[i]->smpl;
        ++J->n_in_smpl[s]; ++RUN.n_reads;
        if (J->lastf_smpl[s] != f) { ++J->nf_smpl[s]; J->lastf_smpl[s] = f; }
    }
    free(keep); free(b);
}
/* Stage 1 of a tile that ends at t1: the reads that start before its pool's end come off the files.  The tile's pool is the reads
 * that overlap the tile widened by `margin` on both sides: the realignment of an indel candidate reads a read's bases and qualities
 * up to INDEL_WINDOW_SIZE columns beyond the tile (bam2bcf_indel.c:38, 174-175), and those qualities carry the mate-overlap tweak
 * of a mate that may lie wholly outside the tile -- so a read's mate has to be in the pool with it.  margin = the longest reference
 * span seen so far + the window; the files are read again when a longer read widened it.  Returns the margin. */
static int read_batch(job_t *J, int t1)
{
    const double tr0 = O.want_timing ? now_s() : 0.;
    int margin = J->max_span + 64, margin_read;
    do {
        margin_read = margin;
        for (int f = 0; f < J->F; ++f) read_file_batch(J, f, t1 + margin);
        margin = J->max_span + 64;
    } while (margin > margin_read);
    if (O.want_timing) RUN.t_read += now_s() - tr0;
    return margin;
}
/* Stage 2: the tile's pool = the reads of the windows that overlap the widened tile, file after file.  Returns its reads. */
static int fill_pool(job_t *J, tilejob_t *T, int t0, int t1, int margin)
{
    const double tp0 = O.want_timing ? now_s() : 0.;
    pool_t *P = &T->P;
    pool_clear(P);
    for (int f = 0; f < J->F; ++f) {
        J->first[f] = P->n;
        for (int i = 0; i < J->win[f].n; ++i) { const lrec_t *x = J->win[f].r[i]; if (overlaps(x->pos, x->end, t0 - margin, t1 + margin)) pool_add_rec(P, f, x); }
    }
    J->first[J->F] = P->n;
    T->S = J->S; T->t0 = t0; T->t1 = t1; T->contig = J->ref_name; T->ref = J->ref; T->ref_len = J->ref_len;
    if (O.want_timing) RUN.t_pool += now_s() - tp0;
    return P->n;
}
/* Reads that end before the next tile's pool begins are through.  Returns where the next tile starts: t1, or further on after a
 * stretch without reads, or reg_end when no file has a read left for the region. */
static int retire_window(job_t *J, int t1, int margin)
{
    int left = 0, next_pos = OPEN_END, more = 0;
    for (int f = 0; f < J->F; ++f) {
        lwin_t *w = &J->win[f];
        int m = 0;
        for (int i = 0; i < w->n; ++i) { lrec_t *x = w->r[i]; if ((x->end == x->pos ? x->pos + 1 : x->end) > t1 - margin) w->r[m++] = x; else lrec_free(x); }
        w->n = m; left += m;
        reader_fetch(&J->rdr[f]);
        if (J->rdr[f].head) { more = 1; if (J->rdr[f].head->pos < next_pos) next_pos = J->rdr[f].head->pos; }
    }
    if (left) return t1;
    if (!more) return reg_end;
    return next_pos - margin > t1 ? next_pos - margin : t1;
}
static void run_region(job_t *J, const region_t *g)
{
    if (!J->ref_name || strcmp(J->ref_name, g->contig)) {
        emit_wait();                                                         /* (the writer may still read the old sequence) */
        free(J->ref); free(J->ref_name);
        J->ref = read_contig(O.ref_path, g->contig, &J->ref_len); J->ref_name = strdup(g->contig);
    }
    reg_beg = g->beg; reg_end = g->end;
    if (reg_end <= reg_beg) return;
    for (int f = 0; f < J->F; ++f) { reader_open(&J->rdr[f], J->kept_path[f]); for (int i = 0; i < J->win[f].n; ++i) lrec_free(J->win[f].r[i]); J->win[f].n = 0; }
    bcfgpu_depth_cap_reset(J->dcap);
    parsers_start(J->rdr, J->sfile, J->F, J->ref_name);
    for (int t0 = reg_beg; t0 < reg_end; ) {
        const int t1 = t0 + O.tile_cols < reg_end ? t0 + O.tile_cols : reg_end;
        const int margin = read_batch(J, t1);
        if (!O.list_only) {
            tilejob_t *T = &TJ[tj_fill];
            if (fill_pool(J, T, t0, t1, margin)) { tile_submit(T, J->first, J->F); ++RUN.n_tiles; }
            else { tile_drain(); emit_wait(); pending_flush(); }            /* columns without a read: a gap ends a gVCF block (gvcf.c:131) */
            RUN.n_cols += (unsigned long long)(t1 - t0);
        }
        t0 = retire_window(J, t1, margin);
    }
    tile_drain();                                                           /* (the next region may bring another reference sequence) */
    parsers_stop(J->rdr, J->F);
    for (int f = 0; f < J->F; ++f) reader_close(&J->rdr[f]);
}
static int report(job_t *J)
{
    if (O.list_only) {
        /* --list-samples: what the host side decided, one line per output sample -- name, reads that enter the pileup, files they
         * come from -- and nothing else (the read-group plumbing, the filters and the depth cap run without a device) */
        for (int s = 0; s < J->S; ++s) printf("%s\t%lld\t%d\n", SM.smpl[s], J->n_in_smpl[s], J->nf_smpl[s]);
        return 0;
    }
    emit_finish();
    pending_flush();
    if (ctx) { uint32_t nw = 0; CHECK(bcfgpu_truncated_cells(ctx, &nw)); RUN.n_wide_cells += nw; }
    if (RUN.n_wide_cells) fprintf(stderr, "[bcfgpu_sam] note: %llu (site, sample) cells of more than 255 usable reads were left to the first-255 rule "
                                          "instead of errmod_cal's draw\n", RUN.n_wide_cells);
    fprintf(stderr, "%llu reads of %d samples, %llu overlapping pairs, %llu pileup entries in %llu columns (%d tiles of <= %d)\n",
            RUN.n_reads, J->S, RUN.tot_pairs, RUN.tot_entries, RUN.n_cols, RUN.n_tiles, O.tile_cols);
    if (O.want_timing) fprintf(stderr, "[bcfgpu_sam] seconds: reading and parsing the files %.3f, tile pools %.3f, device stages %.3f, writing records %.3f, waiting in bcfgpu_pool_adopt %.3f\n", RUN.t_read, RUN.t_pool, RUN.t_dev, RUN.t_emit, RUN.t_adopt);
    if (O.want_timing) fprintf(stderr, "[bcfgpu_sam] device records: %llu records with their FORMAT block encoded on the device\n", RUN.n_dev_records);
    if (O.want_timing && O.device_text) fprintf(stderr, "[bcfgpu_sam] device text: %llu records with their sample columns formatted on the device\n", RUN.n_dev_text);
    if (vio_close(RUN.fout)) DIE("%s\n", vio_error());
    if (ctx) bcfgpu_destroy(ctx);
    if (cap_ctx) bcfgpu_destroy(cap_ctx);
    bcfgpu_depth_cap_free(J->dcap);
    return 0;
}

int main(int argc, char **argv)
{
    job_t J; memset(&J, 0, sizeof J);
    J.argc0 = argc; J.argv0 = argv;
    parse_options(&argc, &argv);
    input_files(&J, argc, argv);
    regions(&J);
    open_inputs(&J);                                                          /* (--list-samples stops in report(): nothing on the way opens the device) */
    if (shard_or_device(&J)) return 0;
    write_header(&J);
    tile_loop_init(&J);
    for (int g = 0; g < J.n_reg; ++g) run_region(&J, &J.reg[g]);
    return report(&J);
}
