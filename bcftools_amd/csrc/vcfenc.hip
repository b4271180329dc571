// vcfenc.hip -- the per-sample part of an mpileup record as VCF text, made on the device: what bcf_call2bcf's
// bcf_update_format_int32 calls (bam2bcf.c:845-903) and the text writer (vcf_format of htslib vcf.c; here host/vcfio.c
// vio_write_record_int, the text branch) do per record on one host thread.  Per sample the record holds a tab, then the FORMAT keys'
// values joined by ':', a key's values joined by ',', every value in decimal: a transposition of the result planes
// ([plane][sample] -> [sample][plane]) with a number of bytes per sample that depends on the values.
//
//   vcf_size_kernel    one workgroup a site: the length of every sample's text, summed to the block's size
//   enc_offsets        the blocks' offsets (the device scan, gather.hip)
//   vcf_write_kernel   one workgroup a site, a lane a sample, in rounds: the lengths again, their exclusive scan over the workgroup,
//                      then every lane formats its sample into LDS at its offset and the round's bytes are stored from there 16 bytes
//                      a lane, consecutive lanes to consecutive addresses, from any byte the block starts at (line_store,
//                      bcfcodec.h).  A round ends with the last sample whose text still lies inside the stage (VCF_STAGE bytes,
//                      not a number of samples); the next round starts at the sample after it.
// The keys, their widths and values are those of bcfenc.hip (bcfcodec.h).
#include <hipcub/hipcub.hpp>
#include "bcfcodec.h"

using namespace bcfgpu;

namespace bcfgpu {

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
static_assert(VCF_STAGE % COD_LINE == 0, "the stage is whole lines");

// bytes of sample s's text at site k: the tab, a ':' between keys, per key a ',' between values and the values' digits.
// keys: bit kind = the key is written (PL, bit 0, always is)
__device__ __forceinline__ int sample_len(const MplpPlanes &P, uint32_t keys, int na, size_t k, int s, size_t S)
{
    int len = 0;
    #pragma unroll
    for (int kind = 0; kind < BCFGPU_BCF_NKEYS; ++kind) {
        if (!(keys >> kind & 1u)) continue;
        const int w = key_width(kind, na);
        len += w;                                               // the tab or ':' in front of the key, w - 1 ','
        for (int j = 0; j < w; ++j) len += n_digits((uint32_t)key_value(P, kind, k, j, s, S));
    }
    return len;
}

// size[k] = bytes of site k's block (0: no record), size[n_sites] = 0
__global__ __launch_bounds__(COD_THREADS) void vcf_size_kernel(MplpPlanes P, uint32_t keys, const uint8_t *emit, int n_sites, int n_smpl,
                                                               unsigned long long *size)
{
    __shared__ unsigned long long red[COD_THREADS / 64];
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= n_sites) { if (tid == 0) size[n_sites] = 0; return; }
    if (emit && !emit[k]) { if (tid == 0) size[k] = 0; return; }
    const int na = site_alleles(P.site[k]);
    const size_t S = (size_t)n_smpl;
    unsigned long long b = 0;
    for (int s = tid; s < n_smpl; s += COD_THREADS) b += (unsigned long long)sample_len(P, keys, na, (size_t)k, s, S);
    for (int d = 32; d; d >>= 1) b += __shfl_xor(b, d, 64);
    if ((tid & 63) == 0) red[tid >> 6] = b;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < COD_THREADS / 64; ++w) t += red[w];
        size[k] = t;
    }
}

__global__ __launch_bounds__(COD_THREADS) void vcf_write_kernel(MplpPlanes P, uint32_t keys, int n_sites, int n_smpl, const unsigned long long *off,
                                                                unsigned char *buf)
{
    typedef hipcub::BlockScan<int, COD_THREADS> Scan;
    __shared__ __attribute__((aligned(16))) unsigned char stage[COD_LINE + VCF_STAGE];
    __shared__ typename Scan::TempStorage scan_tmp;
    __shared__ int round_bytes;
    const int k = blockIdx.x, tid = threadIdx.x;
    if (off[k + 1] == off[k]) return;                                       // no record at this site
    const int na = site_alleles(P.site[k]);
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
        const int sh = line_shift(g);
        // every lane's text into LDS.  Lanes write single bytes at offsets that depend on the values before them: how these
        // conflict on the banks is not measured
        if (in) {
            unsigned char *p = stage + sh + at;
            #pragma unroll
            for (int kind = 0; kind < BCFGPU_BCF_NKEYS; ++kind) {
                if (!(keys >> kind & 1u)) continue;
                const int w = key_width(kind, na);
                for (int j = 0; j < w; ++j) {
                    *p++ = j ? ',' : kind ? ':' : '\t';
                    p = put_value(p, (uint32_t)key_value(P, kind, (size_t)k, j, s, S));
                }
            }
        }
        __syncthreads();
        const int nb = round_bytes;
        line_store(stage, g, nb, tid);
        __syncthreads();
        g += nb; s0 += fit;
    }
}

}  // namespace bcfgpu

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
    if (n_sites == 0) return enc_offsets(ctx, st, "bcfgpu_mplp_encode_vcf", d_off, 1, cap_bytes, n_bytes);
    MplpPlanes P; MplpKeys K;
    if (int rc = mplp_keys("bcfgpu_mplp_encode_vcf", cfg, planes, nullptr, P, K)) return rc;
    uint32_t keys = 0;                                                      // bit kind: the key is written
    for (int i = 0; i < K.n; ++i) keys |= 1u << K.kind[i];
    unsigned long long *off = reinterpret_cast<unsigned long long*>(d_off);
    hipLaunchKernelGGL(vcf_size_kernel, dim3(n_sites + 1), dim3(COD_THREADS), 0, st, P, keys, d_emit, n_sites, S, off);
    const int rc = enc_offsets(ctx, st, "bcfgpu_mplp_encode_vcf", d_off, n_sites + 1, cap_bytes, n_bytes);
    if (rc || *n_bytes == 0) return rc;
    hipLaunchKernelGGL(vcf_write_kernel, dim3(n_sites), dim3(COD_THREADS), 0, st, P, keys, n_sites, S, off, (unsigned char*)d_buf);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_mplp_encode_vcf: write pass");
    return 0;
}
