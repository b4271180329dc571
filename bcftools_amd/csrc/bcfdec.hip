// bcfdec.hip -- the FORMAT vectors mcall() reads from BCF input (PL; AD or QS with -G) as the int32 planes of bcfgpu_call_in, made
// on the device straight from the records' bytes: what bcf_get_format_int32 (mcall.c:1444, :1475) and htslib's unpacking of the
// per-sample block behind it do per record on one host thread.  bcfenc.hip reversed: a key's values of one record are one run of
// n_smpl_in x width little-endian integers of 1, 2 or 4 bytes, sample-major, starting at any byte; the planes want them widened to
// int32 and along samples ([sample][value] -> [plane][sample]).
//
//   bcf_decode_kernel  one workgroup a site: the run in slices of samples -- a slice comes into LDS 16 bytes a lane, consecutive lanes
//                      consecutive addresses, from any byte it starts at (line_load, bcfcodec.h).  Then a lane a called sample:
//                      its values out of LDS, the sentinel rule of the text route (host/vcfio.c dec_int, then the parse of
//                      host/bcfgpu_call.c), 4-byte stores to consecutive addresses of each plane.  The planes past the
//                      record's width are filled in the same pass.
//                      With a sample map (col) the lanes are the called samples and every slice is one pass over them: a lane
//                      whose input sample lies in the slice takes it from LDS, the others wait for theirs.
//                      A sample wider than the stage (width x size > COD_SLICE: no mpileup record) is read from global memory.
#include "bcfcodec.h"

using namespace bcfgpu;

static_assert(sizeof(bcfgpu_bcf_vec) == 16, "bcfgpu_bcf_vec is 16 bytes");

#ifndef BCFDEC_COL_GLOBAL
#define BCFDEC_COL_GLOBAL 0     // 1: with a sample map and more than one slice, lanes read global memory instead of a pass per slice
#endif                          // (the build tools/decode_col_timing.py compares the product with; the product is built with 0)

namespace bcfgpu {

// the planes of one called sample: o = plane 0 at that sample, p = the sample's first value, wr = values to read
__device__ __forceinline__ void dec_sample(int32_t *o, size_t S, int n_planes, const unsigned char *p, int wr, int es, bool aligned)
{
    bool ended = false;
    for (int j = 0; j < n_planes; ++j) {
        int32_t x = BCFGPU_INT32_VECTOR_END;
        if (j < wr && !ended) { x = get_int(p + j * es, es, aligned); ended = x == BCFGPU_INT32_VECTOR_END; }
        if (j == 0 && x == BCFGPU_INT32_VECTOR_END) x = BCFGPU_INT32_MISSING;       // an empty vector is '.'
        o[(size_t)j * S] = x;
    }
}

__global__ __launch_bounds__(COD_THREADS) void bcf_decode_kernel(const unsigned char *indiv, const bcfgpu_bcf_vec *vec, const int32_t *col,
                                                                 int n_smpl_in, int n_smpl, int n_planes, int32_t *out)
{
    __shared__ __attribute__((aligned(16))) unsigned char stage[COD_LINE + COD_SLICE];
    const int k = blockIdx.x, tid = threadIdx.x;
    const bcfgpu_bcf_vec v = vec[k];
    const size_t S = (size_t)n_smpl;
    int32_t *o = out + (size_t)k * n_planes * S;
    const int es = elem_bytes(v.type), w = v.type ? v.width : 0, wr = w < n_planes ? w : n_planes;
    if (wr == 0) {                                                          // no such key, or no values: '.'
        for (int s = tid; s < n_smpl; s += COD_THREADS) dec_sample(o + s, S, n_planes, nullptr, 0, 1, true);
        return;
    }
    const size_t per = (size_t)w * es;                                      // bytes a sample
    const unsigned char *run = indiv + v.off;
    const bool aligned = ((uintptr_t)run & (es - 1)) == 0;                  // per is a multiple of es: every value of the run alike
    const int slice = per > COD_SLICE ? 0 : (int)(COD_SLICE / per);         // samples a slice
    if (slice == 0 || (BCFDEC_COL_GLOBAL && col && slice < n_smpl_in)) {
        for (int s = tid; s < n_smpl; s += COD_THREADS) dec_sample(o + s, S, n_planes, run + (size_t)(col ? col[s] : s) * per, wr, es, aligned);
        return;
    }
    for (int s0 = 0; s0 < n_smpl_in; s0 += slice) {
        const int cs = n_smpl_in - s0 < slice ? n_smpl_in - s0 : slice, nb = cs * (int)per;
        if (!col && s0 >= n_smpl) break;                                    // the input samples past the called ones
        const unsigned char *l = stage + line_load(stage, run + (size_t)s0 * per, nb, tid);
        __syncthreads();
        // Lanes read `per` bytes apart.  By the bank rule (ds_read_b32 and narrower: 32 banks of 4 bytes, the two halves of a
        // wavefront apart) an odd number of dwords a sample -- PL of 1, 2 and 5 alleles as int32 -- is free of conflicts, 6 and
        // 10 dwords meet two lanes on a bank; the narrow types put several lanes on one dword.  Not measured: the plane stores,
        // n_planes x 4 bytes a sample whatever the type, are the larger part of the traffic.
        if (col) {
            for (int s = tid; s < n_smpl; s += COD_THREADS) {
                const int c = col[s] - s0;
                if (c >= 0 && c < cs) dec_sample(o + s, S, n_planes, l + (size_t)c * per, wr, es, aligned);
            }
        } else {
            const int ce = s0 + cs < n_smpl ? cs : n_smpl - s0;
            for (int c = tid; c < ce; c += COD_THREADS) dec_sample(o + s0 + c, S, n_planes, l + (size_t)c * per, wr, es, aligned);
        }
        __syncthreads();
    }
}

}  // namespace bcfgpu

extern "C" int bcfgpu_call_decode_bcf(bcfgpu_ctx *ctx, int32_t n_sites, int32_t n_smpl_in, const void *d_indiv, uint64_t n_indiv_bytes,
                                      const bcfgpu_bcf_vec *vec, const int32_t *col, int32_t n_planes, int32_t *d_out)
{
    if (!ctx || n_sites < 0 || n_smpl_in < 1 || n_planes < 1 || (n_sites && (!vec || !d_out)) || (n_indiv_bytes && !d_indiv))
        return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_decode_bcf: bad arguments");
    hipStream_t st;
    if (bcfgpu_internal_device(ctx, &st, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_decode_bcf: bad context");
    const int S = bcfgpu_internal_cfg(ctx)->n_smpl;
    if (S < 1 || (!col && S > n_smpl_in)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_decode_bcf: more called samples than input samples and no sample map");
    if (col) for (int s = 0; s < S; ++s) if (col[s] < 0 || col[s] >= n_smpl_in) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_decode_bcf: a sample map entry outside the input samples");
    for (int k = 0; k < n_sites; ++k)
        if (vec[k].type < 0 || vec[k].type > 3 || vec[k].width < 0) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_decode_bcf: a vector's type is not 0-3 or its width is negative");
    for (int k = 0; k < n_sites; ++k) {
        if (!vec[k].type) continue;
        const uint64_t bytes = (uint64_t)n_smpl_in * (uint64_t)vec[k].width * (vec[k].type == 3 ? 4u : (unsigned)vec[k].type);     // < 2^64
        if (bytes > n_indiv_bytes || vec[k].off > n_indiv_bytes - bytes) return bcfgpu_set_error(BCFGPU_E_RANGE, "bcfgpu_call_decode_bcf: a vector runs past the end of the bytes");
    }
    if (n_sites == 0) return 0;
    const bcfgpu_bcf_vec *d_vec = (const bcfgpu_bcf_vec*)ws_upload(ctx, WS_COMPACT_BCFDEC_VEC, vec, (size_t)n_sites * sizeof *vec, 64, st);
    const int32_t *d_col = col ? (const int32_t*)ws_upload(ctx, WS_COMPACT_BCFDEC_COL, col, (size_t)S * 4, 64, st) : nullptr;
    if (!d_vec || (col && !d_col)) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_call_decode_bcf: workspace");
    hipLaunchKernelGGL(bcf_decode_kernel, dim3(n_sites), dim3(COD_THREADS), 0, st, (const unsigned char*)d_indiv, d_vec, d_col, n_smpl_in, S, n_planes, d_out);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_decode_bcf: decode pass");
    return 0;
}
