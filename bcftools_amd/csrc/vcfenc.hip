// vcfenc.hip -- the per-sample part of an mpileup record as VCF text, made on the device: what bcf_call2bcf's
// bcf_update_format_int32 calls (bam2bcf.c:845-903) and the text writer (vcf_format of htslib vcf.c; here host/vcfio.c
// vio_write_record_int, the text branch) do per record on one host thread.  Per sample the record holds a tab, then the FORMAT keys'
// values joined by ':', a key's values joined by ',', every value in decimal: a transposition of the result planes
// ([plane][sample] -> [sample][plane]) with a number of bytes per sample that depends on the values.
//
//   vcf_size_kernel    one workgroup a site: the length of every sample's text, summed to the block's size
//   hipcub ExclusiveSum  the blocks' offsets (the scan bcfgpu_mplp_encode_bcf uses, bcfenc.hip)
//   vcf_write_kernel   one workgroup a site, a lane a sample, in rounds: the lengths again, their exclusive scan over the workgroup,
//                      then every lane formats its sample into LDS at its offset and the round's bytes are stored from there 16 bytes
//                      a lane, consecutive lanes to consecutive addresses.  A round ends with the last sample whose text still lies
//                      inside the stage (VCF_STAGE bytes, not a number of samples); the next round starts at the sample after it.  A
//                      block starts at any byte: a round's bytes sit in LDS at the offset their first byte has inside a 16-byte line
//                      of the output, so that the aligned lines of both coincide; the bytes before the first and after the last whole
//                      line go out one by one.
// The keys, their widths and values are those of bcfenc.hip (key_width / key_value are restated here, as in bcfkeys.hip).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <cstdint>
#include "ctx.h"

using namespace bcfgpu;

namespace bcfgpu {

struct TxtPlanes {
    const bcfgpu_site *site;
    const uint8_t *pl, *sp;
    const uint16_t *dp4, *adf, *adr, *scr;
    const int32_t *qs;
};

constexpr int TXT_THREADS = 256;
constexpr int TXT_LINE = 16;                                    // bytes a lane stores at once
constexpr int VCF_STAGE = 15 * 1024;                            // payload bytes of a round in LDS
// the longest text of one sample: the tab, ten ':', and per key its values at their planes' largest (u8 255; u16 65535; DP the sum of
// four u16 = 262140; DV, AD and DPR the sum of two = 131070; QS int32 = 2147483647) with the ',' between them
constexpr int VCF_SAMPLE_MAX = 1 + (BCFGPU_BCF_NKEYS - 1)
                             + (BCFGPU_MAX_PL * 3 + BCFGPU_MAX_PL - 1)                  // PL
                             + 6 + 6 + 3                                                // DP, DV, SP
                             + (4 * 5 + 3)                                              // DP4
                             + 2 * (BCFGPU_MAX_ALLELES * 5 + BCFGPU_MAX_ALLELES - 1)    // ADF, ADR
                             + 2 * (BCFGPU_MAX_ALLELES * 6 + BCFGPU_MAX_ALLELES - 1)    // AD, DPR
                             + 5                                                        // SCR
                             + (BCFGPU_MAX_ALLELES * 10 + BCFGPU_MAX_ALLELES - 1);      // QS
static_assert(VCF_SAMPLE_MAX == 293, "the worst-case sample of eleven keys");
static_assert(VCF_SAMPLE_MAX <= VCF_STAGE, "one sample always fits the stage: every round takes at least one");
static_assert(VCF_STAGE % TXT_LINE == 0, "the stage is whole lines");

__device__ __forceinline__ int txt_key_width(int kind, int na)
{
    switch (kind) {
        case BCFGPU_BCF_PL: return na * (na + 1) / 2;
        case BCFGPU_BCF_DP4: return 4;
        case BCFGPU_BCF_ADF: case BCFGPU_BCF_ADR: case BCFGPU_BCF_AD: case BCFGPU_BCF_DPR: case BCFGPU_BCF_QS: return na;
        default: return 1;                                      // DP, DV, SP, SCR
    }
}

// value j of sample s of the key at site k (bam2bcf.c:845-903: DP and DV are sums of the DP4 counts, AD and DPR of ADF and ADR)
__device__ __forceinline__ uint32_t txt_key_value(const TxtPlanes &P, int kind, size_t k, int j, int s, size_t S)
{
    switch (kind) {
        case BCFGPU_BCF_PL:  return P.pl[(k * BCFGPU_MAX_PL + j) * S + s];
        case BCFGPU_BCF_DP:  { const uint16_t *d = P.dp4 + k * 4 * S + s; return (uint32_t)d[0] + d[S] + d[2 * S] + d[3 * S]; }
        case BCFGPU_BCF_DV:  { const uint16_t *d = P.dp4 + k * 4 * S + s; return (uint32_t)d[2 * S] + d[3 * S]; }
        case BCFGPU_BCF_SP:  return P.sp[k * S + s];
        case BCFGPU_BCF_DP4: return P.dp4[(k * 4 + j) * S + s];
        case BCFGPU_BCF_ADF: return P.adf[(k * 5 + j) * S + s];
        case BCFGPU_BCF_ADR: return P.adr[(k * 5 + j) * S + s];
        case BCFGPU_BCF_AD: case BCFGPU_BCF_DPR: return (uint32_t)P.adf[(k * 5 + j) * S + s] + P.adr[(k * 5 + j) * S + s];
        case BCFGPU_BCF_SCR: return P.scr[k * S + s];
        default:             return (uint32_t)P.qs[(k * 5 + j) * S + s];  // QS (>= 0)
    }
}

__device__ __forceinline__ int txt_site_alleles(const bcfgpu_site &c) { const int na = c.n_alleles; return na < 1 ? 1 : na > BCFGPU_MAX_ALLELES ? BCFGPU_MAX_ALLELES : na; }

// decimal digits of v, by comparisons
__device__ __forceinline__ int n_digits(uint32_t v)
{
    return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u)
             + (v >= 100000000u) + (v >= 1000000000u);
}

// bytes of sample s's text at site k: the tab, a ':' between keys, per key a ',' between values and the values' digits.
// keys: bit kind = the key is written (PL, bit 0, always is)
__device__ __forceinline__ int sample_len(const TxtPlanes &P, uint32_t keys, int na, size_t k, int s, size_t S)
{
    int len = 0;
    #pragma unroll
    for (int kind = 0; kind < BCFGPU_BCF_NKEYS; ++kind) {
        if (!(keys >> kind & 1u)) continue;
        const int w = txt_key_width(kind, na);
        len += w;                                               // the tab or ':' in front of the key, w - 1 ','
        for (int j = 0; j < w; ++j) len += n_digits(txt_key_value(P, kind, k, j, s, S));
    }
    return len;
}

// v in decimal at p (LDS), written from its known end backwards; returns the byte after it
__device__ __forceinline__ unsigned char *put_value(unsigned char *p, uint32_t v)
{
    const int nd = n_digits(v);
    for (int i = nd - 1; i > 0; --i) { const uint32_t q = v / 10u; p[i] = (unsigned char)('0' + (v - q * 10u)); v = q; }
    p[0] = (unsigned char)('0' + v);
    return p + nd;
}

// size[k] = bytes of site k's block (0: no record), size[n_sites] = 0
__global__ __launch_bounds__(TXT_THREADS) void vcf_size_kernel(TxtPlanes P, uint32_t keys, const uint8_t *emit, int n_sites, int n_smpl,
                                                               unsigned long long *size)
{
    __shared__ unsigned long long red[TXT_THREADS / 64];
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= n_sites) { if (tid == 0) size[n_sites] = 0; return; }
    if (emit && !emit[k]) { if (tid == 0) size[k] = 0; return; }
    const int na = txt_site_alleles(P.site[k]);
    const size_t S = (size_t)n_smpl;
    unsigned long long b = 0;
    for (int s = tid; s < n_smpl; s += TXT_THREADS) b += (unsigned long long)sample_len(P, keys, na, (size_t)k, s, S);
    for (int d = 32; d; d >>= 1) b += __shfl_xor(b, d, 64);
    if ((tid & 63) == 0) red[tid >> 6] = b;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < TXT_THREADS / 64; ++w) t += red[w];
        size[k] = t;
    }
}

__global__ __launch_bounds__(TXT_THREADS) void vcf_write_kernel(TxtPlanes P, uint32_t keys, int n_sites, int n_smpl, const unsigned long long *off,
                                                                unsigned char *buf)
{
    typedef hipcub::BlockScan<int, TXT_THREADS> Scan;
    __shared__ __attribute__((aligned(16))) unsigned char stage[TXT_LINE + VCF_STAGE];
    __shared__ typename Scan::TempStorage scan_tmp;
    __shared__ int round_bytes;
    const int k = blockIdx.x, tid = threadIdx.x;
    if (off[k + 1] == off[k]) return;                                       // no record at this site
    const int na = txt_site_alleles(P.site[k]);
    const size_t S = (size_t)n_smpl;
    unsigned char *g = buf + off[k];                                        // where the round's first byte goes
    for (int s0 = 0; s0 < n_smpl; ) {
        // the lengths of up to 256 samples and where each starts in the round; the round ends with the last sample whose text
        // ends inside the stage (the lanes that fit are the first `fit` ones: the ends only grow; lane 0 always fits)
        const int s = s0 + tid;
        const int len = s < n_smpl ? sample_len(P, keys, na, (size_t)k, s, S) : 0;
        int at;
        Scan(scan_tmp).ExclusiveSum(len, at);
        const bool in = s < n_smpl && at + len <= VCF_STAGE;
        const int fit = __syncthreads_count(in);
        if (tid == fit - 1) round_bytes = at + len;
        const int sh = (int)((uintptr_t)g & (TXT_LINE - 1));
        // every lane's text into LDS.  Lanes write single bytes at offsets that depend on the values before them: how these
        // conflict on the banks is not measured
        if (in) {
            unsigned char *p = stage + sh + at;
            #pragma unroll
            for (int kind = 0; kind < BCFGPU_BCF_NKEYS; ++kind) {
                if (!(keys >> kind & 1u)) continue;
                const int w = txt_key_width(kind, na);
                for (int j = 0; j < w; ++j) {
                    *p++ = j ? ',' : kind ? ':' : '\t';
                    p = put_value(p, txt_key_value(P, kind, (size_t)k, j, s, S));
                }
            }
        }
        __syncthreads();
        const int nb = round_bytes;
        // LDS bytes [sh, sh + nb) -> g - sh + the same offsets: whole 16-byte lines in the middle, single bytes at both ends
        const int lo = sh, hi = sh + nb;
        const int l0 = (lo + TXT_LINE - 1) / TXT_LINE, l1 = hi / TXT_LINE;          // whole lines [l0, l1)
        unsigned char *ga = g - sh;
        if (l0 < l1) {
            for (int x = l0 + tid; x < l1; x += TXT_THREADS)
                reinterpret_cast<uint4*>(ga)[x] = reinterpret_cast<const uint4*>(stage)[x];
            const int head = l0 * TXT_LINE - lo, tail = hi - l1 * TXT_LINE;         // each < 16
            if (tid < head) ga[lo + tid] = stage[lo + tid];
            else if (tid >= 32 && tid - 32 < tail) ga[l1 * TXT_LINE + tid - 32] = stage[l1 * TXT_LINE + tid - 32];
        } else {
            for (int x = lo + tid; x < hi; x += TXT_THREADS) ga[x] = stage[x];      // fewer than 31 bytes, no whole line
        }
        __syncthreads();
        g += nb; s0 += fit;
    }
}

}  // namespace bcfgpu

// FORMAT keys of an mpileup record and the flag that selects each, in bcf_call2bcf's order (bam2bcf.c:845-903)
static const int TXT_KEY_FLAG[BCFGPU_BCF_NKEYS] = { 0, BCFGPU_FMT_DP, BCFGPU_FMT_DV, BCFGPU_FMT_SP, BCFGPU_FMT_DP4, BCFGPU_FMT_ADF, BCFGPU_FMT_ADR,
                                                    BCFGPU_FMT_AD, BCFGPU_FMT_DPR, BCFGPU_FMT_SCR, BCFGPU_FMT_QS };

extern "C" int bcfgpu_mplp_encode_vcf(bcfgpu_ctx *ctx, int32_t n_sites, const bcfgpu_mplp_out *planes, const uint8_t *d_emit,
                                      void *d_buf, uint64_t cap_bytes, uint64_t *d_off, uint64_t *n_bytes)
{
    if (!n_bytes) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_mplp_encode_vcf: bad arguments");
    *n_bytes = 0;
    if (!ctx || !planes || !d_off || n_sites < 0 || (cap_bytes && !d_buf)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_mplp_encode_vcf: bad arguments");
    hipStream_t st;
    if (bcfgpu_internal_device(ctx, &st, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_mplp_encode_vcf: bad context");
    const bcfgpu_cfg *cfg = bcfgpu_internal_cfg(ctx);
    const int S = cfg->n_smpl;
    if (n_sites == 0) {
        if (hipMemsetAsync(d_off, 0, sizeof(uint64_t), st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_mplp_encode_vcf: offsets");
        return 0;
    }
    TxtPlanes P = { planes->site, planes->pl, planes->sp, planes->dp4, planes->adf, planes->adr, planes->scr, planes->qs };
    uint32_t keys = 0;
    for (int i = 0; i < BCFGPU_BCF_NKEYS; ++i) {
        if (i != BCFGPU_BCF_PL && !(cfg->fmt_flag & TXT_KEY_FLAG[i])) continue;
        keys |= 1u << i;
        const bool have = i == BCFGPU_BCF_PL ? P.pl != nullptr : i == BCFGPU_BCF_SP ? P.sp != nullptr : i == BCFGPU_BCF_SCR ? P.scr != nullptr :
                          i == BCFGPU_BCF_QS ? P.qs != nullptr : i == BCFGPU_BCF_ADF ? P.adf != nullptr : i == BCFGPU_BCF_ADR ? P.adr != nullptr :
                          (i == BCFGPU_BCF_AD || i == BCFGPU_BCF_DPR) ? P.adf && P.adr : P.dp4 != nullptr;
        if (!have) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_mplp_encode_vcf: a plane the context's fmt_flag asks for is NULL");
    }
    if (!P.site) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_mplp_encode_vcf: no site records");
    uint64_t *h_total = (uint64_t*)bcfgpu_internal_pinned(ctx, PIN_VCF_TOTAL, sizeof(uint64_t));
    if (!h_total) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_mplp_encode_vcf: workspace");
    unsigned long long *off = reinterpret_cast<unsigned long long*>(d_off);
    hipLaunchKernelGGL(vcf_size_kernel, dim3(n_sites + 1), dim3(TXT_THREADS), 0, st, P, keys, d_emit, n_sites, S, off);
    size_t tmp = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, off, off, n_sites + 1, st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_mplp_encode_vcf: scan");
    void *d_tmp = bcfgpu_internal_ws(ctx, WS_COMPACT_VCF_SCAN_TMP, tmp + 64);
    if (!d_tmp) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_mplp_encode_vcf: workspace");
    if (hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp, off, off, n_sites + 1, st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_mplp_encode_vcf: scan");
    if (hipMemcpyAsync(h_total, off + n_sites, sizeof(uint64_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_mplp_encode_vcf: size pass");
    *n_bytes = *h_total;
    // the blocks do not fit: nothing is written, the caller learns the size and may come back with a larger buffer
    if (*n_bytes > cap_bytes) return bcfgpu_set_error(BCFGPU_E_RANGE, "bcfgpu_mplp_encode_vcf: the buffer is too small for the blocks (n_bytes tells the size)");
    if (*n_bytes == 0) return 0;
    hipLaunchKernelGGL(vcf_write_kernel, dim3(n_sites), dim3(TXT_THREADS), 0, st, P, keys, n_sites, S, off, (unsigned char*)d_buf);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_mplp_encode_vcf: write pass");
    return 0;
}
