// bcfenc.hip -- the per-sample part of an mpileup record as BCF2 bytes, made on the device: what bcf_call2bcf's
// bcf_update_format_int32 calls (bam2bcf.c:845-903) and the writer's typed-value encoder (bcf_enc_vint of htslib vcf.c; here
// host/vcfio.c enc_int1 / enc_size / enc_vint) do per record on one host thread.  Per FORMAT key the "indiv" block of a record holds
// a typed key id, a type / length descriptor and n_smpl x width little-endian integers, sample-major, in the smallest of
// int8 / int16 / int32 that holds the key's values at that site: a transposition of the result planes ([plane][sample] ->
// [sample][plane]) with a range reduction.
//
//   bcf_size_kernel    one workgroup a site: the maximum of every key's values -> the key's integer type, the block's size
//   enc_offsets        the blocks' offsets (the device scan bcfgpu_compact_calls uses, gather.hip)
//   bcf_write_kernel   one workgroup a site: per key the header bytes, then the values in slices of samples -- read from the planes
//                      along samples (consecutive lanes, consecutive samples), put into LDS at their place in the record, and stored
//                      from there 16 bytes a lane, consecutive lanes to consecutive addresses, from any byte the block starts at.
//                      The copy out of LDS is line_store (bcfcodec.h); the keys, their widths and values are bcfcodec.h's too.
#include "bcfcodec.h"

using namespace bcfgpu;

namespace bcfgpu {

// size[k] = bytes of site k's block (0: no record), size[n_sites] = 0; types[k] = the keys' BCF2 integer types (1, 2, 3), two bits a key
__global__ __launch_bounds__(COD_THREADS) void bcf_size_kernel(MplpPlanes P, MplpKeys K, const uint8_t *emit, int n_sites, int n_smpl,
                                                               unsigned long long *size, uint32_t *types)
{
    __shared__ int32_t red[COD_THREADS / 64][BCFGPU_BCF_NKEYS];
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
            for (int s = tid; s < n_smpl; s += COD_THREADS)
                for (int j = 0; j < w; ++j) { const int32_t v = key_value(P, kind, (size_t)k, j, s, S); m[i] = v > m[i] ? v : m[i]; }
        }
    }
    wg_max(m, red, tid);
    if (tid == 0) {
        unsigned long long b = 0; uint32_t ty = 0;
        #pragma unroll
        for (int i = 0; i < BCFGPU_BCF_NKEYS; ++i) {
            if (i >= K.n) continue;
            const int t = int_type(m[i], 0), w = key_width(K.kind[i], na);
            ty |= (uint32_t)t << (2 * i);
            b += (unsigned long long)(id_bytes(K.id[i]) + desc_bytes(w)) + (unsigned long long)S * (unsigned)w * (unsigned)elem_bytes(t);
        }
        size[k] = b; types[k] = ty;
    }
}

__global__ __launch_bounds__(COD_THREADS) void bcf_write_kernel(MplpPlanes P, MplpKeys K, int n_sites, int n_smpl, const unsigned long long *off,
                                                                const uint32_t *types, unsigned char *buf)
{
    __shared__ __attribute__((aligned(16))) unsigned char stage[COD_LINE + COD_SLICE];
    const int k = blockIdx.x, tid = threadIdx.x;
    if (off[k + 1] == off[k]) return;                                       // no record at this site
    const int na = site_alleles(P.site[k]);
    const size_t S = (size_t)n_smpl;
    const uint32_t ty = types[k];
    unsigned char *dst = buf + off[k];
    for (int i = 0; i < K.n; ++i) {
        const int kind = K.kind[i], id = K.id[i], w = key_width(kind, na), t = (int)(ty >> (2 * i) & 3u), es = elem_bytes(t);
        if (tid == 0) put_header(dst, id, w, t);
        dst += id_bytes(id) + desc_bytes(w);
        const int per = w * es, slice = COD_SLICE / per;                    // bytes a sample, samples a slice (>= 256)
        for (int s0 = 0; s0 < n_smpl; s0 += slice) {
            const int cs = n_smpl - s0 < slice ? n_smpl - s0 : slice, nb = cs * per;
            unsigned char *g = dst + (size_t)s0 * per;                      // where the slice's first byte goes
            const int sh = line_shift(g);
            unsigned char *l = stage + sh;
            // the values of the slice, transposed into LDS.  Lanes write `per` bytes apart: by the bank rule (32 banks of 4 bytes
            // for writes) a 2- to 4-way conflict at strides of 8 and 16 bytes (DP4 as int16 / int32); not measured
            if (sh % es == 0) {
                for (int s = tid; s < cs; s += COD_THREADS)
                    for (int j = 0; j < w; ++j) put_int<false>(l + (s * w + j) * es, (uint32_t)key_value(P, kind, (size_t)k, j, s0 + s, S), es);
            } else {                                                        // values that straddle their natural alignment: byte by byte
                for (int s = tid; s < cs; s += COD_THREADS)
                    for (int j = 0; j < w; ++j) put_int<true>(l + (s * w + j) * es, (uint32_t)key_value(P, kind, (size_t)k, j, s0 + s, S), es);
            }
            __syncthreads();
            line_store(stage, g, nb, tid);
            __syncthreads();
        }
        dst += S * (size_t)per;
    }
}

}  // namespace bcfgpu

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
    if (n_sites == 0) return enc_offsets(ctx, st, "bcfgpu_mplp_encode_bcf", d_off, 1, cap_bytes, n_bytes);
    MplpPlanes P; MplpKeys K;
    if (int rc = mplp_keys("bcfgpu_mplp_encode_bcf", cfg, planes, key_id, P, K)) return rc;
    uint32_t *d_types = (uint32_t*)bcfgpu_internal_ws(ctx, WS_COMPACT_BCF_TYPES, (size_t)n_sites * 4 + 64);
    if (!d_types) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_mplp_encode_bcf: workspace");
    unsigned long long *off = reinterpret_cast<unsigned long long*>(d_off);
    hipLaunchKernelGGL(bcf_size_kernel, dim3(n_sites + 1), dim3(COD_THREADS), 0, st, P, K, d_emit, n_sites, S, off, d_types);
    const int rc = enc_offsets(ctx, st, "bcfgpu_mplp_encode_bcf", d_off, n_sites + 1, cap_bytes, n_bytes);
    if (rc || *n_bytes == 0) return rc;
    hipLaunchKernelGGL(bcf_write_kernel, dim3(n_sites), dim3(COD_THREADS), 0, st, P, K, n_sites, S, off, d_types, (unsigned char*)d_buf);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_mplp_encode_bcf: write pass");
    return 0;
}
