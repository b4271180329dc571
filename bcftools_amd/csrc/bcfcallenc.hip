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
//   hipcub ExclusiveSum  the blocks' offsets, one per site and key
//   callbcf_write_kernel one workgroup a site: per key the header bytes, then the values in slices of samples -- read from the
//                        planes along samples, put into LDS at their place in the record, and stored from there 16 bytes a lane.
//                        A block starts at any byte: a slice sits in LDS at the offset its first byte has inside a 16-byte line
//                        of the output; the bytes before the first and after the last whole line go out one by one.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <cstdint>
#include "ctx.h"

using namespace bcfgpu;

namespace bcfgpu {

struct CallEncPlanes {
    const bcfgpu_call_site *site;
    const int8_t *gt;
    const int32_t *pl, *gq;
    int n_gt_max;
};
struct CallEncIds { int id[BCFGPU_CALL_BCF_NKEYS]; };

constexpr int CENC_THREADS = 256;
constexpr int CENC_LINE = 16;                                   // bytes a lane stores at once
constexpr int CENC_SLICE = BCFGPU_MAX_PL * 4 * 256;             // payload bytes of a slice in LDS: 256 samples of a 15-wide int32 PL
constexpr int CENC_NRED = 6;                                    // GT width 2?, PL width, PL max, -PL min, GQ max, -GQ min
constexpr int32_t CENC_NONE = INT32_MIN + 1;                    // "no value yet" of a maximum (enc_vint starts there)

__device__ __forceinline__ int cenc_id_bytes(int id) { return id <= 127 ? 2 : id <= 32767 ? 3 : 5; }      // a typed scalar: descriptor + value
__device__ __forceinline__ int cenc_desc_bytes(int w) { return w < 15 ? 1 : 3; }                         // width >= 15: 0xF?, then the width as a typed int8
__device__ __forceinline__ int cenc_nals(const bcfgpu_call_site &c) { const int nn = c.nals_new; return nn < 1 ? 1 : nn > BCFGPU_MAX_ALLELES ? BCFGPU_MAX_ALLELES : nn; }
__device__ __forceinline__ int cenc_type(int32_t mx, int32_t neg_mn) { return mx <= 127 && neg_mn <= 120 ? 1 : mx <= 32767 && neg_mn <= 32760 ? 2 : 3; }
// the packed word of a site: bits 0-1 GT's type (0: no GT), 2-3 PL's (0: absent), 4-5 GQ's (0: absent), 6-7 GT's width, 8-11 PL's
__device__ __forceinline__ uint32_t cenc_pack(int tgt, int tpl, int tgq, int wgt, int wpl) { return (uint32_t)tgt | (uint32_t)tpl << 2 | (uint32_t)tgq << 4 | (uint32_t)wgt << 6 | (uint32_t)wpl << 8; }
// a plane's value as the integer of `es` bytes that stands for it: the sentinels are the type's own, not the int32's low bytes
__device__ __forceinline__ uint32_t cenc_narrow(int32_t v, int es)
{
    if (es == 4 || (v != BCFGPU_INT32_MISSING && v != BCFGPU_INT32_VECTOR_END)) return (uint32_t)v;
    return (es == 1 ? 0x80u : 0x8000u) | (uint32_t)(v == BCFGPU_INT32_VECTOR_END);
}

// size[3k + i] = bytes of key i's block of site k (0: absent, or no record), size[3 n_sites] = 0; word[k] = cenc_pack(...)
__global__ __launch_bounds__(CENC_THREADS) void callbcf_size_kernel(CallEncPlanes P, CallEncIds K, const uint8_t *emit, int n_sites, int n_smpl,
                                                                    unsigned long long *size, uint32_t *word)
{
    __shared__ int32_t red[CENC_THREADS / 64][CENC_NRED];
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= n_sites) { if (tid == 0) size[(size_t)n_sites * BCFGPU_CALL_BCF_NKEYS] = 0; return; }
    unsigned long long *sz = size + (size_t)k * BCFGPU_CALL_BCF_NKEYS;
    if (emit && !emit[k]) { if (tid == 0) { sz[0] = sz[1] = sz[2] = 0; word[k] = 0; } return; }
    const bcfgpu_call_site c = P.site[k];
    const int nn = cenc_nals(c);
    int ngn = nn * (nn + 1) / 2; if (ngn > P.n_gt_max) ngn = P.n_gt_max;
    const bool has_pl = P.pl && !c.pl_dropped, has_gq = P.gq && nn > 1 && c.ret > 0;
    const size_t S = (size_t)n_smpl;
    int32_t m[CENC_NRED] = { 0, 0, CENC_NONE, CENC_NONE, CENC_NONE, CENC_NONE };
    for (int s = tid; s < n_smpl; s += CENC_THREADS) {
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
    #pragma unroll
    for (int i = 0; i < CENC_NRED; ++i)
        for (int d = 32; d; d >>= 1) { const int32_t o = __shfl_xor(m[i], d, 64); m[i] = o > m[i] ? o : m[i]; }
    if ((tid & 63) == 0) {
        #pragma unroll
        for (int i = 0; i < CENC_NRED; ++i) red[tid >> 6][i] = m[i];
    }
    __syncthreads();
    if (tid == 0) {
        #pragma unroll
        for (int i = 0; i < CENC_NRED; ++i)
            for (int w = 1; w < CENC_THREADS / 64; ++w) m[i] = red[w][i] > m[i] ? red[w][i] : m[i];
        const int wgt = 1 + m[0], wpl = has_pl ? m[1] : 0;
        const int tpl = has_pl ? cenc_type(m[2], m[3]) : 0, tgq = has_gq ? cenc_type(m[4], m[5]) : 0;
        sz[BCFGPU_CALL_BCF_GT] = (unsigned long long)(cenc_id_bytes(K.id[BCFGPU_CALL_BCF_GT]) + 1) + (unsigned long long)S * (unsigned)wgt;
        sz[BCFGPU_CALL_BCF_PL] = !has_pl ? 0 : (unsigned long long)(cenc_id_bytes(K.id[BCFGPU_CALL_BCF_PL]) + cenc_desc_bytes(wpl)) + (unsigned long long)S * (unsigned)wpl * (tpl == 3 ? 4u : (unsigned)tpl);
        sz[BCFGPU_CALL_BCF_GQ] = !has_gq ? 0 : (unsigned long long)(cenc_id_bytes(K.id[BCFGPU_CALL_BCF_GQ]) + 1) + (unsigned long long)S * (tgq == 3 ? 4u : (unsigned)tgq);
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
            v = cenc_narrow(x, es);
        } else v = cenc_narrow(P.gq[k * S + s], es);
        unsigned char *o = q + j * es;
        if (BYTEWISE) { for (int b = 0; b < es; ++b) o[b] = (unsigned char)(v >> (8 * b)); }
        else if (es == 1) *o = (unsigned char)v;
        else if (es == 2) *reinterpret_cast<uint16_t*>(o) = (uint16_t)v;
        else *reinterpret_cast<uint32_t*>(o) = v;
    }
}

__global__ __launch_bounds__(CENC_THREADS) void callbcf_write_kernel(CallEncPlanes P, CallEncIds K, int n_sites, int n_smpl, const unsigned long long *off,
                                                                     const uint32_t *word, unsigned char *buf)
{
    __shared__ __attribute__((aligned(16))) unsigned char stage[CENC_LINE + CENC_SLICE];
    const int k = blockIdx.x, tid = threadIdx.x;
    const unsigned long long *ok = off + (size_t)k * BCFGPU_CALL_BCF_NKEYS;
    if (ok[BCFGPU_CALL_BCF_NKEYS] == ok[0]) return;                         // no record at this site
    const uint32_t wd = word[k];
    const int nn = cenc_nals(P.site[k]);
    int ngn = nn * (nn + 1) / 2; if (ngn > P.n_gt_max) ngn = P.n_gt_max;
    const size_t S = (size_t)n_smpl;
    for (int i = 0; i < BCFGPU_CALL_BCF_NKEYS; ++i) {
        if (ok[i + 1] == ok[i]) continue;                                   // the key is absent at this site
        const int id = K.id[i], t = (int)(wd >> (2 * i) & 3u), es = t == 3 ? 4 : t;
        const int w = i == BCFGPU_CALL_BCF_GT ? (int)(wd >> 6 & 3u) : i == BCFGPU_CALL_BCF_PL ? (int)(wd >> 8 & 15u) : 1;
        unsigned char *dst = buf + ok[i];
        if (tid == 0) {                                                     // typed key id, then the type / length descriptor
            unsigned char *h = dst;
            if (id <= 127) { h[0] = 0x11; h[1] = (unsigned char)id; h += 2; }
            else if (id <= 32767) { h[0] = 0x12; h[1] = (unsigned char)(id & 0xff); h[2] = (unsigned char)(id >> 8); h += 3; }
            else { h[0] = 0x13; h[1] = (unsigned char)(id & 0xff); h[2] = (unsigned char)(id >> 8 & 0xff); h[3] = (unsigned char)(id >> 16 & 0xff); h[4] = (unsigned char)(id >> 24 & 0xff); h += 5; }
            if (w < 15) h[0] = (unsigned char)(w << 4 | t);
            else { h[0] = (unsigned char)(0xF0 | t); h[1] = 0x11; h[2] = (unsigned char)w; }
        }
        dst += cenc_id_bytes(id) + cenc_desc_bytes(w);
        const int per = w * es, slice = CENC_SLICE / per;                   // bytes a sample, samples a slice (>= 256)
        for (int s0 = 0; s0 < n_smpl; s0 += slice) {
            const int cs = n_smpl - s0 < slice ? n_smpl - s0 : slice, nb = cs * per;
            unsigned char *g = dst + (size_t)s0 * per;                      // where the slice's first byte goes
            const int sh = (int)((uintptr_t)g & (CENC_LINE - 1));
            unsigned char *l = stage + sh;
            // the values of the slice, transposed into LDS.  Lanes write `per` bytes apart.  By the bank rule (32 banks of 4 bytes
            // for writes, lanes in groups of 32) a sample of d dwords is gcd(d, 32)-way: an int32 PL of 1, 3 or 15 values (the
            // 60 bytes of five alleles) is free of conflicts, one of 6 or 10 values 2-way; below 4 bytes a sample (GT, GQ as
            // int8 / int16, a narrow PL) neighbouring lanes write into one dword; not measured
            if (sh % es == 0) {
                for (int s = tid; s < cs; s += CENC_THREADS) cenc_put_sample<false>(P, i, (size_t)k, s0 + s, S, w, es, ngn, l + (size_t)s * per);
            } else {                                                        // values that straddle their natural alignment: byte by byte
                for (int s = tid; s < cs; s += CENC_THREADS) cenc_put_sample<true>(P, i, (size_t)k, s0 + s, S, w, es, ngn, l + (size_t)s * per);
            }
            __syncthreads();
            // LDS bytes [sh, sh + nb) -> g - sh + the same offsets: whole 16-byte lines in the middle, single bytes at both ends
            const int lo = sh, hi = sh + nb;
            const int l0 = (lo + CENC_LINE - 1) / CENC_LINE, l1 = hi / CENC_LINE;   // whole lines [l0, l1)
            unsigned char *ga = g - sh;
            if (l0 < l1) {
                for (int x = l0 + tid; x < l1; x += CENC_THREADS)
                    reinterpret_cast<uint4*>(ga)[x] = reinterpret_cast<const uint4*>(stage)[x];
                const int head = l0 * CENC_LINE - lo, tail = hi - l1 * CENC_LINE;   // each < 16
                if (tid < head) ga[lo + tid] = stage[lo + tid];
                else if (tid >= 32 && tid - 32 < tail) ga[l1 * CENC_LINE + tid - 32] = stage[l1 * CENC_LINE + tid - 32];
            } else {
                for (int x = lo + tid; x < hi; x += CENC_THREADS) ga[x] = stage[x];  // fewer than 31 bytes, no whole line
            }
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
    if (n_sites == 0) {
        if (hipMemsetAsync(d_off, 0, sizeof(uint64_t), st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_encode_bcf: offsets");
        return 0;
    }
    if (!planes->site || !planes->gt) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_bcf: no site records or no genotypes");
    CallEncPlanes P = { planes->site, planes->gt, planes->pl, planes->gq, n_gt_max };
    CallEncIds K;
    for (int i = 0; i < BCFGPU_CALL_BCF_NKEYS; ++i) {
        if (key_id[i] < 0) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_bcf: negative key id");
        K.id[i] = key_id[i];
    }
    const int n_off = n_sites * BCFGPU_CALL_BCF_NKEYS + 1;
    uint32_t *d_word = (uint32_t*)bcfgpu_internal_ws(ctx, WS_COMPACT_BCFCALL_WORD, (size_t)n_sites * 4 + 64);
    uint64_t *h_total = (uint64_t*)bcfgpu_internal_pinned(ctx, PIN_BCFCALL_TOTAL, sizeof(uint64_t));
    if (!d_word || !h_total) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_call_encode_bcf: workspace");
    unsigned long long *off = reinterpret_cast<unsigned long long*>(d_off);
    hipLaunchKernelGGL(callbcf_size_kernel, dim3(n_sites + 1), dim3(CENC_THREADS), 0, st, P, K, d_emit, n_sites, S, off, d_word);
    size_t tmp = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, off, off, n_off, st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_encode_bcf: scan");
    void *d_tmp = bcfgpu_internal_ws(ctx, WS_COMPACT_BCFCALL_SCAN_TMP, tmp + 64);
    if (!d_tmp) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_call_encode_bcf: workspace");
    if (hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp, off, off, n_off, st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_encode_bcf: scan");
    if (hipMemcpyAsync(h_total, off + n_off - 1, sizeof(uint64_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_encode_bcf: size pass");
    *n_bytes = *h_total;
    // the blocks do not fit: nothing is written, the caller learns the size and may come back with a larger buffer
    if (*n_bytes > cap_bytes) return bcfgpu_set_error(BCFGPU_E_RANGE, "bcfgpu_call_encode_bcf: the buffer is too small for the blocks (n_bytes tells the size)");
    if (*n_bytes == 0) return 0;
    hipLaunchKernelGGL(callbcf_write_kernel, dim3(n_sites), dim3(CENC_THREADS), 0, st, P, K, n_sites, S, off, d_word, (unsigned char*)d_buf);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_encode_bcf: write pass");
    return 0;
}
