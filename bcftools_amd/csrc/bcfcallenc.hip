// bcfcallenc.hip -- the per-sample part of a call record as BCF2 bytes, made on the device: FORMAT/GT, the trimmed FORMAT/PL and
// FORMAT/GQ of the records mcall() leaves (mcall.c:1158-1194 the trimmed PL, :1583 PL dropped, :1618-1623 GQ / GP on called
// variant records), what bcf_update_genotypes / bcf_update_format_int32 and the writer's typed-value encoder (bcf_enc_vint of
// htslib vcf.c; here host/vcfio.c enc_vint) do per record on one host thread.  The mirror of bcfenc.hip for the caller's planes,
// which carry what the mpileup planes never do:
//   GT   a byte plane of allele indices -> (allele + 1) << 1, missing -> 0; two values a sample when any sample of the record has
//        two, a haploid sample's second then being int8's `end of vector`; always int8
//   PL   an int32 plane with `missing` / `end of vector` sentinels: a sample's vector is its leading values up to its first `end of
//        vector` (none: one `missing`), the record's width the longest of them -- the haploid samples of a diploid record are
//        padded, an all-haploid record is nals wide --, the type from the largest and the smallest value that is no sentinel
//        (enc_vint's rule: int8 holds -120 .. 127, int16 -32760 .. 32767); absent when the site has pl_dropped
//   GQ   one int32 a sample, `missing` kept; only on records with more than one allele that were called (ret > 0)
// Every key's block is complete in itself (typed key id, descriptor, values) and has an offset of its own, so that the host can
// put other keys' blocks between them.
//
//   callbcf_size_kernel  one workgroup a site: per sample the PL vector's length, over the samples the widths, the largest and
//                        smallest values (wavefront shuffles, then LDS) -> the keys' types and sizes, one packed word a site
//   enc_offsets          the blocks' offsets, one per site and key (the device scan, gather.hip)
//   callbcf_write_kernel one workgroup a site: per key the header bytes, then the values in slices of samples -- read from the
//                        planes along samples, put into LDS at their place in the record, and stored from there 16 bytes a lane,
//                        from any byte the block starts at (line_store, bcfcodec.h).
#include "bcfcodec.h"

using namespace bcfgpu;

namespace bcfgpu {

struct CallEncPlanes {
    const bcfgpu_call_site *site;
    const int8_t *gt;
    const int32_t *pl, *gq;
    int n_gt_max;
};
struct CallEncIds { int id[BCFGPU_CALL_BCF_NKEYS]; };

constexpr int CENC_NRED = 6;                                    // GT width 2?, PL width, PL max, -PL min, GQ max, -GQ min

__device__ __forceinline__ int cenc_nals(const bcfgpu_call_site &c) { const int nn = c.nals_new; return nn < 1 ? 1 : nn > BCFGPU_MAX_ALLELES ? BCFGPU_MAX_ALLELES : nn; }
// the packed word of a site: bits 0-1 GT's type (0: no GT), 2-3 PL's (0: absent), 4-5 GQ's (0: absent), 6-7 GT's width, 8-11 PL's
__device__ __forceinline__ uint32_t cenc_pack(int tgt, int tpl, int tgq, int wgt, int wpl) { return (uint32_t)tgt | (uint32_t)tpl << 2 | (uint32_t)tgq << 4 | (uint32_t)wgt << 6 | (uint32_t)wpl << 8; }
// size[3k + i] = bytes of key i's block of site k (0: absent, or no record), size[3 n_sites] = 0; word[k] = cenc_pack(...)
__global__ __launch_bounds__(COD_THREADS) void callbcf_size_kernel(CallEncPlanes P, CallEncIds K, const uint8_t *emit, int n_sites, int n_smpl,
                                                                    unsigned long long *size, uint32_t *word)
{
    __shared__ int32_t red[COD_THREADS / 64][CENC_NRED];
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= n_sites) { if (tid == 0) size[(size_t)n_sites * BCFGPU_CALL_BCF_NKEYS] = 0; return; }
    unsigned long long *sz = size + (size_t)k * BCFGPU_CALL_BCF_NKEYS;
    if (emit && !emit[k]) { if (tid == 0) { sz[0] = sz[1] = sz[2] = 0; word[k] = 0; } return; }
    const bcfgpu_call_site c = P.site[k];
    const int nn = cenc_nals(c);
    int ngn = nn * (nn + 1) / 2; if (ngn > P.n_gt_max) ngn = P.n_gt_max;
    const bool has_pl = P.pl && !c.pl_dropped, has_gq = P.gq && nn > 1 && c.ret > 0;
    const size_t S = (size_t)n_smpl;
    int32_t m[CENC_NRED] = { 0, 0, COD_NONE, COD_NONE, COD_NONE, COD_NONE };
    for (int s = tid; s < n_smpl; s += COD_THREADS) {
        m[0] |= P.gt[((size_t)k * 2 + 1) * S + s] != BCFGPU_GT_VECTOR_END;
        if (has_pl) {
            const int32_t *p = P.pl + (size_t)k * P.n_gt_max * S + s;
            int len = 0;
            for (; len < ngn; ++len) {
                const int32_t v = p[(size_t)len * S];
                if (v == BCFGPU_INT32_VECTOR_END) break;
                if (v == BCFGPU_INT32_MISSING) continue;
                m[2] = v > m[2] ? v : m[2]; m[3] = -v > m[3] ? -v : m[3];
            }
            if (len < 1) len = 1;                               // no value at all: one `missing`
            m[1] = len > m[1] ? len : m[1];
        }
        if (has_gq) {
            const int32_t v = P.gq[(size_t)k * S + s];
            if (v != BCFGPU_INT32_MISSING && v != BCFGPU_INT32_VECTOR_END) { m[4] = v > m[4] ? v : m[4]; m[5] = -v > m[5] ? -v : m[5]; }
        }
    }
    wg_max(m, red, tid);
    if (tid == 0) {
        const int wgt = 1 + m[0], wpl = has_pl ? m[1] : 0;
        const int tpl = has_pl ? int_type(m[2], m[3]) : 0, tgq = has_gq ? int_type(m[4], m[5]) : 0;
        sz[BCFGPU_CALL_BCF_GT] = (unsigned long long)(id_bytes(K.id[BCFGPU_CALL_BCF_GT]) + 1) + (unsigned long long)S * (unsigned)wgt;
        sz[BCFGPU_CALL_BCF_PL] = !has_pl ? 0 : (unsigned long long)(id_bytes(K.id[BCFGPU_CALL_BCF_PL]) + desc_bytes(wpl)) + (unsigned long long)S * (unsigned)wpl * (unsigned)elem_bytes(tpl);
        sz[BCFGPU_CALL_BCF_GQ] = !has_gq ? 0 : (unsigned long long)(id_bytes(K.id[BCFGPU_CALL_BCF_GQ]) + 1) + (unsigned long long)S * (unsigned)elem_bytes(tgq);
        word[k] = cenc_pack(1, tpl, tgq, wgt, wpl);
    }
}

// the w values of sample s of key `kind` at site k, as the integers of `es` bytes the record holds, into q[0 .. w * es) (any alignment
// when bytewise)
template <bool BYTEWISE>
__device__ __forceinline__ void cenc_put_sample(const CallEncPlanes &P, int kind, size_t k, int s, size_t S, int w, int es, int ngn, unsigned char *q)
{
    bool ended = false;                                         // PL: behind the sample's first `end of vector`
    for (int j = 0; j < w; ++j) {
        uint32_t v;
        if (kind == BCFGPU_CALL_BCF_GT) {
            const int g = P.gt[(k * 2 + j) * S + s];
            v = g == BCFGPU_GT_VECTOR_END ? (j ? 0x81u : 0u) : g == BCFGPU_GT_MISSING ? 0u : (uint32_t)(g + 1) << 1;
        } else if (kind == BCFGPU_CALL_BCF_PL) {
            int32_t x = ended || j >= ngn ? BCFGPU_INT32_VECTOR_END : P.pl[(k * P.n_gt_max + j) * S + s];
            if (x == BCFGPU_INT32_VECTOR_END) { ended = true; if (j == 0) x = BCFGPU_INT32_MISSING; }
            v = narrow(x, es);
        } else v = narrow(P.gq[k * S + s], es);
        put_int<BYTEWISE>(q + j * es, v, es);
    }
}

__global__ __launch_bounds__(COD_THREADS) void callbcf_write_kernel(CallEncPlanes P, CallEncIds K, int n_sites, int n_smpl, const unsigned long long *off,
                                                                     const uint32_t *word, unsigned char *buf)
{
    __shared__ __attribute__((aligned(16))) unsigned char stage[COD_LINE + COD_SLICE];
    const int k = blockIdx.x, tid = threadIdx.x;
    const unsigned long long *ok = off + (size_t)k * BCFGPU_CALL_BCF_NKEYS;
    if (ok[BCFGPU_CALL_BCF_NKEYS] == ok[0]) return;                         // no record at this site
    const uint32_t wd = word[k];
    const int nn = cenc_nals(P.site[k]);
    int ngn = nn * (nn + 1) / 2; if (ngn > P.n_gt_max) ngn = P.n_gt_max;
    const size_t S = (size_t)n_smpl;
    for (int i = 0; i < BCFGPU_CALL_BCF_NKEYS; ++i) {
        if (ok[i + 1] == ok[i]) continue;                                   // the key is absent at this site
        const int id = K.id[i], t = (int)(wd >> (2 * i) & 3u), es = elem_bytes(t);
        const int w = i == BCFGPU_CALL_BCF_GT ? (int)(wd >> 6 & 3u) : i == BCFGPU_CALL_BCF_PL ? (int)(wd >> 8 & 15u) : 1;
        unsigned char *dst = buf + ok[i];
        if (tid == 0) put_header(dst, id, w, t);
        dst += id_bytes(id) + desc_bytes(w);
        const int per = w * es, slice = COD_SLICE / per;                   // bytes a sample, samples a slice (>= 256)
        for (int s0 = 0; s0 < n_smpl; s0 += slice) {
            const int cs = n_smpl - s0 < slice ? n_smpl - s0 : slice, nb = cs * per;
            unsigned char *g = dst + (size_t)s0 * per;                      // where the slice's first byte goes
            const int sh = line_shift(g);
            unsigned char *l = stage + sh;
            // the values of the slice, transposed into LDS.  Lanes write `per` bytes apart.  By the bank rule (32 banks of 4 bytes
            // for writes, lanes in groups of 32) a sample of d dwords is gcd(d, 32)-way: an int32 PL of 1, 3 or 15 values (the
            // 60 bytes of five alleles) is free of conflicts, one of 6 or 10 values 2-way; below 4 bytes a sample (GT, GQ as
            // int8 / int16, a narrow PL) neighbouring lanes write into one dword; not measured
            if (sh % es == 0) {
                for (int s = tid; s < cs; s += COD_THREADS) cenc_put_sample<false>(P, i, (size_t)k, s0 + s, S, w, es, ngn, l + (size_t)s * per);
            } else {                                                        // values that straddle their natural alignment: byte by byte
                for (int s = tid; s < cs; s += COD_THREADS) cenc_put_sample<true>(P, i, (size_t)k, s0 + s, S, w, es, ngn, l + (size_t)s * per);
            }
            __syncthreads();
            line_store(stage, g, nb, tid);
            __syncthreads();
        }
    }
}

}  // namespace bcfgpu

extern "C" int bcfgpu_call_encode_bcf(bcfgpu_ctx *ctx, int32_t n_sites, int32_t n_gt_max, const bcfgpu_call_out *planes, const int32_t *key_id,
                                      const uint8_t *d_emit, void *d_buf, uint64_t cap_bytes, uint64_t *d_off, uint64_t *n_bytes)
{
    if (!n_bytes) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_bcf: bad arguments");
    *n_bytes = 0;
    if (!ctx || !planes || !key_id || !d_off || n_sites < 0 || n_gt_max < 1 || n_gt_max > BCFGPU_MAX_PL || (cap_bytes && !d_buf))
        return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_bcf: bad arguments");
    if ((uint64_t)n_sites * BCFGPU_CALL_BCF_NKEYS + 1 > (uint64_t)INT32_MAX) return bcfgpu_set_error(BCFGPU_E_RANGE, "bcfgpu_call_encode_bcf: too many sites for one call");
    hipStream_t st;
    if (bcfgpu_internal_device(ctx, &st, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_bcf: bad context");
    const int S = bcfgpu_internal_cfg(ctx)->n_smpl;
    if (n_sites == 0) return enc_offsets(ctx, st, "bcfgpu_call_encode_bcf", d_off, 1, cap_bytes, n_bytes);
    if (!planes->site || !planes->gt) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_bcf: no site records or no genotypes");
    CallEncPlanes P = { planes->site, planes->gt, planes->pl, planes->gq, n_gt_max };
    CallEncIds K;
    for (int i = 0; i < BCFGPU_CALL_BCF_NKEYS; ++i) {
        if (key_id[i] < 0) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_bcf: negative key id");
        K.id[i] = key_id[i];
    }
    const int n_off = n_sites * BCFGPU_CALL_BCF_NKEYS + 1;
    uint32_t *d_word = (uint32_t*)bcfgpu_internal_ws(ctx, WS_COMPACT_BCFCALL_WORD, (size_t)n_sites * 4 + 64);
    if (!d_word) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_call_encode_bcf: workspace");
    unsigned long long *off = reinterpret_cast<unsigned long long*>(d_off);
    hipLaunchKernelGGL(callbcf_size_kernel, dim3(n_sites + 1), dim3(COD_THREADS), 0, st, P, K, d_emit, n_sites, S, off, d_word);
    const int rc = enc_offsets(ctx, st, "bcfgpu_call_encode_bcf", d_off, n_off, cap_bytes, n_bytes);
    if (rc || *n_bytes == 0) return rc;
    hipLaunchKernelGGL(callbcf_write_kernel, dim3(n_sites), dim3(COD_THREADS), 0, st, P, K, n_sites, S, off, d_word, (unsigned char*)d_buf);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_encode_bcf: write pass");
    return 0;
}
