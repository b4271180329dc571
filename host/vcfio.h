/*  vcfio.h -- VCF headers and VCF / BCF2 record streams for the host drivers: what htslib's vcf.c does on the pipe
 *  boundary of `bcftools mpileup | bcftools call` (hts_open / bcf_hdr_write / bcf_write of mpileup.c:502-602,288-316 and
 *  vcfcall.c:703-710; output modes of version.c:67-82).  Host-side record I/O only: nothing here computes.
 *
 *  The drivers build and consume records as VCF text lines; this module frames them:
 *      'v' plain VCF, 'z' bgzip-compressed VCF, 'u' uncompressed BCF2 (BGZF blocks of stored data), 'b' compressed BCF2.
 *  BCF2 records are encoded from / decoded to the text line with the header's dictionaries, following the BCF2.2
 *  specification (typed values, smallest integer type that holds a vector, string dictionary in header order with
 *  PASS = 0, contig dictionary in header order).
 */
#ifndef VCFIO_H
#define VCFIO_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

typedef struct vio_hdr vio_hdr;
typedef struct vio_file vio_file;

/* ---- header ---- */
vio_hdr *vio_hdr_new(void);                                     /* ##fileformat=VCFv4.2 + FILTER PASS, as bcf_hdr_init("w") */
vio_hdr *vio_hdr_parse(const char *text, size_t len);           /* meta lines + #CHROM line */
void vio_hdr_free(vio_hdr *h);
int  vio_hdr_append(vio_hdr *h, const char *line);              /* one "##..." line (with or without the newline) */
int  vio_hdr_remove(vio_hdr *h, const char *kind, const char *id);   /* kind: "INFO", "FORMAT", "FILTER"; the dictionary keeps the id */
int  vio_hdr_add_sample(vio_hdr *h, const char *name);
int  vio_hdr_subset(vio_hdr *h, int n, const int *keep);        /* the samples keep[0..n) of the current list, in that order */
int  vio_hdr_nsamples(const vio_hdr *h);
const char *vio_hdr_sample(const vio_hdr *h, int i);
char *vio_hdr_text(const vio_hdr *h, size_t *len);              /* malloc'ed: every meta line and the #CHROM line */
int  vio_hdr_nlines(const vio_hdr *h);
const char *vio_hdr_line(const vio_hdr *h, int i);              /* meta line i (no newline) */

/* ---- streams ---- */
vio_file *vio_open_write(const char *path, char mode);          /* path "-" = stdout; mode 'v', 'z', 'u' or 'b' */
int  vio_write_hdr(vio_file *f, const vio_hdr *h);
int  vio_write_line(vio_file *f, const vio_hdr *h, const char *line);   /* one VCF record as text, without the newline */
/* A record whose per-sample columns are integers, handed over as arrays instead of text: `head` = the first nine columns (CHROM .. FORMAT,
 * tab separated, no newline); for the k-th FORMAT key the n_samples x width[k] values vals[k][s * width[k] + j] (VIO_INT_VEND after a sample's
 * last value, VIO_INT_MISSING for '.').  The same bytes as vio_write_line of the full text line, as VCF and as BCF -- without a number being
 * printed and parsed back on the way into a BCF record. */
#define VIO_INT_MISSING INT32_MIN
#define VIO_INT_VEND    (INT32_MIN + 1)
int  vio_write_record_int(vio_file *f, const vio_hdr *h, const char *head, int n_keys, const int *width, const int32_t *const *vals);
/* The dictionary index encode_record writes for FORMAT key `id` (what a device-side encoder puts in front of the key's values), or -1
 * when the header declares no such FORMAT key. */
int  vio_hdr_fmt_id(const vio_hdr *h, const char *id);
/* The Type the header declares for the FORMAT key at dictionary index `dict` (vio_indiv_key.dict, vio_hdr_fmt_id): VIO_TYPE_*, or -1
 * when the index is outside the dictionary or no FORMAT line declares the key.  What a writer needs to know before it takes a key's
 * stored integers for integers (bcfgpu_call_remap_bcf), or parses a key's text as integers (bcfgpu_call_parse_keys_vcf). */
enum { VIO_TYPE_FLAG = 0, VIO_TYPE_INT = 1, VIO_TYPE_FLOAT = 2, VIO_TYPE_STR = 3 };
int  vio_hdr_fmt_type(const vio_hdr *h, int dict);
/* A BCF record whose per-sample part is encoded already (bcfgpu_mplp_encode_bcf): `head` as for vio_write_record_int -- the shared part
 * is encoded from it as for every other record, n_fmt being the number of keys in its FORMAT column and n_sample the header's --, then
 * the l_indiv bytes of `indiv` as they are.  BCF output only: -1 on a text file. */
int  vio_write_record_indiv(vio_file *f, const vio_hdr *h, const char *head, const void *indiv, size_t l_indiv);
/* The mirror for text: a VCF record whose sample columns are formatted already (bcfgpu_mplp_encode_vcf): `head` as for
 * vio_write_record_int, then the l_text bytes of `text` ("\t...\t...", what vio_write_record_int's text branch appends after the head)
 * as they are, then the newline.  Text output ('v', 'z') only: -1 with a message on a BCF file. */
int  vio_write_record_text(vio_file *f, const vio_hdr *h, const char *head, const void *text, size_t l_text);
/* FORMAT keys as BCF2 key blocks, without a record around them: `fmt` = the keys as in a FORMAT column ("AD:DP"), `samples` = the
 * n_sample sample columns holding those keys' values, tab separated ("1,2:3\t0,0:1"; a column that ends early has '.' for the rest).
 * Every key's block -- typed key id, descriptor, values, exactly the bytes vio_write_line puts into a record's per-sample part for that
 * key -- is appended to *out (a malloc'ed buffer that grows, *cap its size; overwritten from its start); key_end[k] = the bytes of
 * *out up to and including key k's block (room for 64).  The number of keys, or -1.  A writer that has other keys' blocks ready
 * (bcfgpu_call_encode_bcf; bcfgpu_call_remap_bcf or, on text input, bcfgpu_call_parse_keys_vcf for the integer keys it passes through)
 * puts these between them and hands the whole to vio_write_record_indiv: `fmt` and `samples` then hold only the keys left to the host. */
int  vio_encode_keys(const vio_hdr *h, const char *fmt, const char *samples, int n_sample, char **out, size_t *cap, size_t *key_end);
vio_file *vio_open_read(const char *path);                      /* path "-" = stdin; VCF, bgzipped VCF or BCF2, detected */
vio_hdr *vio_read_hdr(vio_file *f);
int  vio_is_bcf(const vio_file *f);                             /* 1: the stream holds BCF2 records, 0: VCF text */
int  vio_read_line(vio_file *f, const vio_hdr *h, char **line, size_t *cap);   /* 1: a record (as VCF text) in *line, 0: end, <0: error */
/* A BCF record without its sample text: vio_read_line up to and including the FORMAT column (the first nine fields; eight when the
 * file has no samples) in *head, and the record's raw per-sample block where it lies in the file's buffer -- *indiv, *l_indiv bytes,
 * valid until the next read -- with the counts it is read with.  BCF input only: -1 with a message on a text stream.
 * vio_indiv_keys: the n_fmt key headers of such a block (at most 64), truncation checked as vio_read_line checks it; the number of keys
 * filled in, or -1.  vio_indiv_text: the sample columns of the block as text ("\t...\t..."), exactly the bytes vio_read_line puts
 * behind the FORMAT column: head + text is its line. */
typedef struct {
    int dict;               /* the key's index in the header's dictionary */
    const char *id;         /* its name (the header's string) */
    int type, width;        /* BCF2 type code (1 int8, 2 int16, 3 int32, 5 float, 7 char) and values a sample */
    size_t off;             /* byte offset inside the block of value [sample 0][0] */
} vio_indiv_key;
int  vio_read_record(vio_file *f, const vio_hdr *h, char **head, size_t *cap, const void **indiv, size_t *l_indiv, int *n_fmt, int *n_sample);
int  vio_indiv_keys(const vio_hdr *h, const void *indiv, size_t l_indiv, int n_fmt, int n_sample, vio_indiv_key *keys);
int  vio_indiv_text(const vio_hdr *h, const void *indiv, size_t l_indiv, int n_fmt, int n_sample, char **text, size_t *cap);
int  vio_close(vio_file *f);
const char *vio_error(void);

#endif
