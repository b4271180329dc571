/*  drv.h -- what the drivers over the C-ABI share: error exits, the clock, device buffers, the size-then-write
 *  call of the device encoders, the -g limits and -- in a driver that includes vcfio.h first -- the memory stream a
 *  text record is written into.  Static inline, plain C99; the clock needs _POSIX_C_SOURCE >= 199309L. */
#ifndef DRV_H
#define DRV_H
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <time.h>
#include "bcfgpu.h"

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: %s (%d)\n", #call, bcfgpu_last_error(), rc_); exit(1); } } while (0)
#define DIE(...) do { fprintf(stderr, __VA_ARGS__); exit(1); } while (0)
#if defined(_POSIX_C_SOURCE) && _POSIX_C_SOURCE >= 199309L
static inline double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
#endif

static inline void *dev_alloc(bcfgpu_ctx *ctx, size_t bytes)          /* zeroed */
{
    void *p = NULL;
    CHECK(bcfgpu_malloc(ctx, bytes ? bytes : 16, &p));
    CHECK(bcfgpu_memset(ctx, p, 0, bytes ? bytes : 16));
    return p;
}
static inline void *dev_upload(bcfgpu_ctx *ctx, const void *src, size_t bytes)
{
    void *d = NULL;
    CHECK(bcfgpu_malloc(ctx, bytes ? bytes : 16, &d));
    if (bytes) CHECK(bcfgpu_memcpy_h2d(ctx, d, src, bytes));
    return d;
}
/* A device encoder, called twice: without a buffer it tells the bytes it needs (0, or BCFGPU_E_RANGE and *need), with one in HBM it
 * writes them and n_off offsets.  Both come back in malloc'ed host arrays; one sync, and the device buffers are freed. */
typedef int (*encode_fn)(void *arg, void *d_buf, uint64_t cap, uint64_t *d_off, uint64_t *need);
static inline void encode_two_pass(bcfgpu_ctx *ctx, encode_fn fn, void *arg, const char *entry, size_t n_off, unsigned char **bytes, uint64_t **off)
{
    void *d_off = NULL, *d_buf = NULL; uint64_t need = 0;
    CHECK(bcfgpu_malloc(ctx, n_off * 8, &d_off));
    int rc = fn(arg, NULL, 0, d_off, &need);
    if (rc && rc != BCFGPU_E_RANGE) DIE("%s: %s (%d)\n", entry, bcfgpu_last_error(), rc);
    *bytes = malloc(need ? need : 1); *off = malloc(n_off * 8);
    if (need) {
        CHECK(bcfgpu_malloc(ctx, need, &d_buf));
        if ((rc = fn(arg, d_buf, need, d_off, &need))) DIE("%s: %s (%d)\n", entry, bcfgpu_last_error(), rc);
        CHECK(bcfgpu_memcpy_d2h(ctx, *bytes, d_buf, need));
    }
    CHECK(bcfgpu_memcpy_d2h(ctx, *off, d_off, n_off * 8));
    CHECK(bcfgpu_sync(ctx));
    if (d_buf) CHECK(bcfgpu_free(ctx, d_buf));
    CHECK(bcfgpu_free(ctx, d_off));
}
/* -g INT,...: the depth limits of the gVCF blocks (gvcf_init, gvcf.c:47-73).  How many there are, or -1: not a number, an empty
 * item or more than 16 of them (the caller words the error). */
static inline int parse_gvcf_limits(const char *arg, int32_t out[16])
{
    for (int n = 0;; ++arg) {
        char *e; const long v = strtol(arg, &e, 10);
        if (e == arg || (*e && *e != ',') || n == 16) return -1;
        out[n++] = (int32_t)v;
        if (!*e) return n;
        arg = e;
    }
}

#ifdef VCFIO_H
static FILE *LN; static char *ln_buf; static size_t ln_len;      /* the record being written: a memory stream, framed by vcfio */
static inline void open_record_stream(void) { LN = open_memstream(&ln_buf, &ln_len); if (!LN) DIE("open_memstream failed\n"); }
/* the head of a record whose samples reach the writer as bytes or arrays: NUL-terminated in ln_buf; what is written next lies at
 * the offset returned.  The caller hands ln_buf to the writer and rewinds. */
static inline long end_head(void) { fputc(0, LN); fflush(LN); return ftell(LN); }
/* a text record: NUL-terminated, through the writer, then the stream starts over */
static inline void end_record(vio_file *fout, vio_hdr *hdr) { end_head(); if (vio_write_line(fout, hdr, ln_buf)) DIE("%s\n", vio_error()); rewind(LN); }
#endif
#endif
