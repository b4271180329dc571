// bcfenc.hip -- the per-sample part of an mpileup record as BCF2 bytes, made on the device: what bcf_call2bcf's
// bcf_update_format_int32 calls (bam2bcf.c:845-903) and the writer's typed-value encoder (bcf_enc_vint of htslib vcf.c; here
// host/vcfio.c enc_int1 / enc_size / enc_vint) do per record on one host thread.  Per FORMAT key the "indiv" block of a record holds
// a typed key id, a type / length descriptor and n_smpl x width little-endian integers, sample-major, in the smallest of
// int8 / int16 / int32 that holds the key's values at that site: a transposition of the result planes ([plane][sample] ->
// [sample][plane]) with a range reduction.
//
//   bcf_size_kernel    one workgroup a site: the maximum of every key's values -> the key's integer type, the block's size
//   hipcub ExclusiveSum  the blocks' offsets (the scan bcfgpu_compact_calls uses, gather.hip)
//   bcf_write_kernel   one workgroup a site: per key the header bytes, then the values in slices of samples -- read from the planes
//                      along samples (consecutive lanes, consecutive samples), put into LDS at their place in the record, and stored
//                      from there 16 bytes a lane, consecutive lanes to consecutive addresses.  A block starts at any byte: a slice
//                      sits in LDS at the offset its first byte has inside a 16-byte line of the output, so that the aligned
//                      lines of both coincide; the bytes before the first and after the last whole line go out one by one.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <cstdint>
#include "ctx.h"

using namespace bcfgpu;

namespace bcfgpu {

struct EncPlanes {
    const bcfgpu_site *site;
    const uint8_t *pl, *sp;
    const uint16_t *dp4, *adf, *adr, *scr;
    const int32_t *qs;
};
// the keys a record holds, in the order they are written: kind = BCFGPU_BCF_*, id = the writer's dictionary index
struct EncKeys { int n; int kind[BCFGPU_BCF_NKEYS]; int id[BCFGPU_BCF_NKEYS]; };

constexpr int ENC_THREADS = 256;
constexpr int ENC_LINE = 16;                                    // bytes a lane stores at once
constexpr int ENC_SLICE = BCFGPU_MAX_PL * 4 * 256;              // payload bytes of a slice in LDS: 256 samples of the widest key as int32

__device__ __forceinline__ int key_width(int kind, int na)
{
    switch (kind) {
        case BCFGPU_BCF_PL: return na * (na + 1) / 2;
        case BCFGPU_BCF_DP4: return 4;
        case BCFGPU_BCF_ADF: case BCFGPU_BCF_ADR: case BCFGPU_BCF_AD: case BCFGPU_BCF_DPR: case BCFGPU_BCF_QS: return na;
        default: return 1;                                      // DP, DV, SP, SCR
    }
}

// value j of sample s of the key at site k (bam2bcf.c:845-903: DP and DV are sums of the DP4 counts, AD and DPR of ADF and ADR)
__device__ __forceinline__ int32_t key_value(const EncPlanes &P, int kind, size_t k, int j, int s, size_t S)
{
    switch (kind) {
        case BCFGPU_BCF_PL:  return P.pl[(k * BCFGPU_MAX_PL + j) * S + s];
        case BCFGPU_BCF_DP:  { const uint16_t *d = P.dp4 + k * 4 * S + s; return (int32_t)d[0] + d[S] + d[2 * S] + d[3 * S]; }
        case BCFGPU_BCF_DV:  { const uint16_t *d = P.dp4 + k * 4 * S + s; return (int32_t)d[2 * S] + d[3 * S]; }
        case BCFGPU_BCF_SP:  return P.sp[k * S + s];
        case BCFGPU_BCF_DP4: return P.dp4[(k * 4 + j) * S + s];
        case BCFGPU_BCF_ADF: return P.adf[(k * 5 + j) * S + s];
        case BCFGPU_BCF_ADR: return P.adr[(k * 5 + j) * S + s];
        case BCFGPU_BCF_AD: case BCFGPU_BCF_DPR: return (int32_t)P.adf[(k * 5 + j) * S + s] + P.adr[(k * 5 + j) * S + s];
        case BCFGPU_BCF_SCR: return P.scr[k * S + s];
        default:             return P.qs[(k * 5 + j) * S + s];  // QS
    }
}

__device__ __forceinline__ int site_alleles(const bcfgpu_site &c) { const int na = c.n_alleles; return na < 1 ? 1 : na > BCFGPU_MAX_ALLELES ? BCFGPU_MAX_ALLELES : na; }
__device__ __forceinline__ int id_bytes(int id) { return id <= 127 ? 2 : id <= 32767 ? 3 : 5; }          // a typed scalar: descriptor + value
__device__ __forceinline__ int desc_bytes(int w) { return w < 15 ? 1 : 3; }                            // width >= 15: 0xF?, then the width as a typed int8

// size[k] = bytes of site k's block (0: no record), size[n_sites] = 0; types[k] = the keys' BCF2 integer types (1, 2, 3), two bits a key
__global__ __launch_bounds__(ENC_THREADS) void bcf_size_kernel(EncPlanes P, EncKeys K, const uint8_t *emit, int n_sites, int n_smpl,
                                                               unsigned long long *size, uint32_t *types)
{
    __shared__ int32_t red[ENC_THREADS / 64][BCFGPU_BCF_NKEYS];
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= n_sites) { if (tid == 0) size[n_sites] = 0; return; }
    if (emit && !emit[k]) { if (tid == 0) { size[k] = 0; types[k] = 0; } return; }
    const int na = site_alleles(P.site[k]);
    const size_t S = (size_t)n_smpl;
    int32_t m[BCFGPU_BCF_NKEYS];
    #pragma unroll
    for (int i = 0; i < BCFGPU_BCF_NKEYS; ++i) {
        m[i] = 0;
        if (i < K.n) {
            const int kind = K.kind[i], w = key_width(kind, na);
            for (int s = tid; s < n_smpl; s += ENC_THREADS)
                for (int j = 0; j < w; ++j) { const int32_t v = key_value(P, kind, (size_t)k, j, s, S); m[i] = v > m[i] ? v : m[i]; }
            for (int d = 32; d; d >>= 1) { const int32_t o = __shfl_xor(m[i], d, 64); m[i] = o > m[i] ? o : m[i]; }
        }
    }
    if ((tid & 63) == 0) {
        #pragma unroll
        for (int i = 0; i < BCFGPU_BCF_NKEYS; ++i) red[tid >> 6][i] = m[i];
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long b = 0; uint32_t ty = 0;
        for (int i = 0; i < K.n; ++i) {
            int32_t mx = red[0][i];
            for (int w2 = 1; w2 < ENC_THREADS / 64; ++w2) mx = red[w2][i] > mx ? red[w2][i] : mx;
            const int t = mx <= 127 ? 1 : mx <= 32767 ? 2 : 3, w = key_width(K.kind[i], na);
            ty |= (uint32_t)t << (2 * i);
            b += (unsigned long long)(id_bytes(K.id[i]) + desc_bytes(w)) + (unsigned long long)S * (unsigned)w * (t == 3 ? 4u : (unsigned)t);
        }
        size[k] = b; types[k] = ty;
    }
}

__global__ __launch_bounds__(ENC_THREADS) void bcf_write_kernel(EncPlanes P, EncKeys K, int n_sites, int n_smpl, const unsigned long long *off,
                                                                const uint32_t *types, unsigned char *buf)
{
    __shared__ __attribute__((aligned(16))) unsigned char stage[ENC_LINE + ENC_SLICE];
    const int k = blockIdx.x, tid = threadIdx.x;
    if (off[k + 1] == off[k]) return;                                       // no record at this site
    const int na = site_alleles(P.site[k]);
    const size_t S = (size_t)n_smpl;
    const uint32_t ty = types[k];
    unsigned char *dst = buf + off[k];
    for (int i = 0; i < K.n; ++i) {
        const int kind = K.kind[i], id = K.id[i], w = key_width(kind, na), t = (int)(ty >> (2 * i) & 3u), es = t == 3 ? 4 : t;
        if (tid == 0) {                                                     // typed key id, then the type / length descriptor
            unsigned char *h = dst;
            if (id <= 127) { h[0] = 0x11; h[1] = (unsigned char)id; h += 2; }
            else if (id <= 32767) { h[0] = 0x12; h[1] = (unsigned char)(id & 0xff); h[2] = (unsigned char)(id >> 8); h += 3; }
            else { h[0] = 0x13; h[1] = (unsigned char)(id & 0xff); h[2] = (unsigned char)(id >> 8 & 0xff); h[3] = (unsigned char)(id >> 16 & 0xff); h[4] = (unsigned char)(id >> 24 & 0xff); h += 5; }
            if (w < 15) h[0] = (unsigned char)(w << 4 | t);
            else { h[0] = (unsigned char)(0xF0 | t); h[1] = 0x11; h[2] = (unsigned char)w; }
        }
        dst += id_bytes(id) + desc_bytes(w);
        const int per = w * es, slice = ENC_SLICE / per;                    // bytes a sample, samples a slice (>= 256)
        for (int s0 = 0; s0 < n_smpl; s0 += slice) {
            const int cs = n_smpl - s0 < slice ? n_smpl - s0 : slice, nb = cs * per;
            unsigned char *g = dst + (size_t)s0 * per;                      // where the slice's first byte goes
            const int sh = (int)((uintptr_t)g & (ENC_LINE - 1));
            unsigned char *l = stage + sh;
            // the values of the slice, transposed into LDS.  Lanes write `per` bytes apart: by the bank rule (32 banks of 4 bytes
            // for writes) a 2- to 4-way conflict at strides of 8 and 16 bytes (DP4 as int16 / int32); not measured
            if (sh % es == 0) {
                for (int s = tid; s < cs; s += ENC_THREADS)
                    for (int j = 0; j < w; ++j) {
                        const int32_t v = key_value(P, kind, (size_t)k, j, s0 + s, S);
                        unsigned char *q = l + (s * w + j) * es;
                        if (es == 1) *q = (unsigned char)v; else if (es == 2) *reinterpret_cast<uint16_t*>(q) = (uint16_t)v; else *reinterpret_cast<int32_t*>(q) = v;
                    }
            } else {                                                        // values that straddle their natural alignment: byte by byte
                for (int s = tid; s < cs; s += ENC_THREADS)
                    for (int j = 0; j < w; ++j) {
                        const uint32_t v = (uint32_t)key_value(P, kind, (size_t)k, j, s0 + s, S);
                        unsigned char *q = l + (s * w + j) * es;
                        for (int b = 0; b < es; ++b) q[b] = (unsigned char)(v >> (8 * b));
                    }
            }
            __syncthreads();
            // LDS bytes [sh, sh + nb) -> g - sh + the same offsets: whole 16-byte lines in the middle, single bytes at both ends
            const int lo = sh, hi = sh + nb;
            const int l0 = (lo + ENC_LINE - 1) / ENC_LINE, l1 = hi / ENC_LINE;      // whole lines [l0, l1)
            unsigned char *ga = g - sh;
            if (l0 < l1) {
                for (int x = l0 + tid; x < l1; x += ENC_THREADS)
                    reinterpret_cast<uint4*>(ga)[x] = reinterpret_cast<const uint4*>(stage)[x];
                const int head = l0 * ENC_LINE - lo, tail = hi - l1 * ENC_LINE;     // each < 16
                if (tid < head) ga[lo + tid] = stage[lo + tid];
                else if (tid >= 32 && tid - 32 < tail) ga[l1 * ENC_LINE + tid - 32] = stage[l1 * ENC_LINE + tid - 32];
            } else {
                for (int x = lo + tid; x < hi; x += ENC_THREADS) ga[x] = stage[x];  // fewer than 31 bytes, no whole line
            }
            __syncthreads();
        }
        dst += S * (size_t)per;
    }
}

}  // namespace bcfgpu

// FORMAT keys of an mpileup record and the flag that selects each, in bcf_call2bcf's order (bam2bcf.c:845-903)
static const int KEY_FLAG[BCFGPU_BCF_NKEYS] = { 0, BCFGPU_FMT_DP, BCFGPU_FMT_DV, BCFGPU_FMT_SP, BCFGPU_FMT_DP4, BCFGPU_FMT_ADF, BCFGPU_FMT_ADR,
                                                BCFGPU_FMT_AD, BCFGPU_FMT_DPR, BCFGPU_FMT_SCR, BCFGPU_FMT_QS };

extern "C" int bcfgpu_mplp_encode_bcf(bcfgpu_ctx *ctx, int32_t n_sites, const bcfgpu_mplp_out *planes, const int32_t *key_id,
                                      const uint8_t *d_emit, void *d_buf, uint64_t cap_bytes, uint64_t *d_off, uint64_t *n_bytes)
{
    if (!n_bytes) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_mplp_encode_bcf: bad arguments");
    *n_bytes = 0;
    if (!ctx || !planes || !key_id || !d_off || n_sites < 0 || (cap_bytes && !d_buf)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_mplp_encode_bcf: bad arguments");
    hipStream_t st;
    if (bcfgpu_internal_device(ctx, &st, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_mplp_encode_bcf: bad context");
    const bcfgpu_cfg *cfg = bcfgpu_internal_cfg(ctx);
    const int S = cfg->n_smpl;
    if (n_sites == 0) {
        if (hipMemsetAsync(d_off, 0, sizeof(uint64_t), st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_mplp_encode_bcf: offsets");
        return 0;
    }
    EncPlanes P = { planes->site, planes->pl, planes->sp, planes->dp4, planes->adf, planes->adr, planes->scr, planes->qs };
    EncKeys K; K.n = 0;
    for (int i = 0; i < BCFGPU_BCF_NKEYS; ++i) {
        if (i != BCFGPU_BCF_PL && !(cfg->fmt_flag & KEY_FLAG[i])) continue;
        if (key_id[i] < 0) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_mplp_encode_bcf: negative key id");
        K.kind[K.n] = i; K.id[K.n] = key_id[i]; ++K.n;
        const bool have = i == BCFGPU_BCF_PL ? P.pl != nullptr : i == BCFGPU_BCF_SP ? P.sp != nullptr : i == BCFGPU_BCF_SCR ? P.scr != nullptr :
                          i == BCFGPU_BCF_QS ? P.qs != nullptr : i == BCFGPU_BCF_ADF ? P.adf != nullptr : i == BCFGPU_BCF_ADR ? P.adr != nullptr :
                          (i == BCFGPU_BCF_AD || i == BCFGPU_BCF_DPR) ? P.adf && P.adr : P.dp4 != nullptr;
        if (!have) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_mplp_encode_bcf: a plane the context's fmt_flag asks for is NULL");
    }
    if (!P.site) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_mplp_encode_bcf: no site records");
    uint32_t *d_types = (uint32_t*)bcfgpu_internal_ws(ctx, WS_COMPACT_BCF_TYPES, (size_t)n_sites * 4 + 64);
    uint64_t *h_total = (uint64_t*)bcfgpu_internal_pinned(ctx, PIN_BCF_TOTAL, sizeof(uint64_t));
    if (!d_types || !h_total) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_mplp_encode_bcf: workspace");
    unsigned long long *off = reinterpret_cast<unsigned long long*>(d_off);
    hipLaunchKernelGGL(bcf_size_kernel, dim3(n_sites + 1), dim3(ENC_THREADS), 0, st, P, K, d_emit, n_sites, S, off, d_types);
    size_t tmp = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, off, off, n_sites + 1, st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_mplp_encode_bcf: scan");
    void *d_tmp = bcfgpu_internal_ws(ctx, WS_COMPACT_BCF_SCAN_TMP, tmp + 64);
    if (!d_tmp) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_mplp_encode_bcf: workspace");
    if (hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp, off, off, n_sites + 1, st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_mplp_encode_bcf: scan");
    if (hipMemcpyAsync(h_total, off + n_sites, sizeof(uint64_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_mplp_encode_bcf: size pass");
    *n_bytes = *h_total;
    // the blocks do not fit: nothing is written, the caller learns the size and may come back with a larger buffer
    if (*n_bytes > cap_bytes) return bcfgpu_set_error(BCFGPU_E_RANGE, "bcfgpu_mplp_encode_bcf: the buffer is too small for the blocks (n_bytes tells the size)");
    if (*n_bytes == 0) return 0;
    hipLaunchKernelGGL(bcf_write_kernel, dim3(n_sites), dim3(ENC_THREADS), 0, st, P, K, n_sites, S, off, d_types, (unsigned char*)d_buf);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_mplp_encode_bcf: write pass");
    return 0;
}
