// vcfdec.hip -- the FORMAT vectors mcall() reads from VCF text input (PL; AD or QS with -G) as the int32 planes of bcfgpu_call_in,
// made on the device straight from the records' sample columns: what vcf_parse_format and the bcf_get_format_int32 calls behind
// mcall.c:1444 and :1475 do per record on one host thread (here: the splits and atoi of host/bcfgpu_call.c build_planes).
// vcfenc.hip / vcfcallenc.hip reversed: a record's columns are one run of text, a tab in front of every column, the columns of any
// length; the planes want one field of every column as integers along samples.
//
//   vcfdec_index_kernel  one workgroup a site: the run through the LDS stage in slices (line_load, bcfcodec.h), a lane four 16-byte
//                        lines of it: the tabs of its lines counted, the counts' exclusive scan over the workgroup and a running
//                        base across slices give every tab its ordinal, and the tab's offset inside the run goes to
//                        start[site][ordinal]; start[site][n_smpl_in] = the run's length.  A run that does not begin with a tab or
//                        does not hold n_smpl_in of them puts its site into the error word (the smallest such site).  Without
//                        `start` the kernel only counts: the check of a call that fills the slot more than once.
//   vcfdec_parse_kernel  one workgroup a site, a lane a called sample.  Without a sample map in rounds cut by bytes: the columns of
//                        up to 256 samples are one span of the run; a round ends with the last sample whose text still lies inside
//                        the stage, the span comes into LDS by line_load, and every lane walks its column there: idx colons
//                        skipped, the values parsed, 4-byte stores along samples into every plane, `end of vector` behind the
//                        vector in the same pass.  A column longer than the stage is read from global memory by one lane.
//                        With a sample map (col) the lanes read their columns from global memory, in rounds of 256.
#include <hipcub/hipcub.hpp>
#include "bcfcodec.h"

using namespace bcfgpu;

static_assert(sizeof(bcfgpu_vcf_vec) == 16, "bcfgpu_vcf_vec is 16 bytes");
static_assert(BCFGPU_VCFDEC_START_BYTES % 4 == 0, "the offsets are u32");

namespace bcfgpu {

constexpr int VDEC_LANE_LINES = 4;                              // lines a lane of the index kernel looks at in a slice
static_assert((COD_LINE + COD_SLICE + COD_LINE - 1) / COD_LINE <= VDEC_LANE_LINES * COD_THREADS, "the lanes' lines cover the stage");
static_assert(COD_SLICE % COD_LINE == 0, "the stage is whole lines");

__global__ __launch_bounds__(COD_THREADS) void vcfdec_index_kernel(const unsigned char *text, const bcfgpu_vcf_vec *vec, int k0, int n_smpl_in,
                                                                   uint32_t *start, uint32_t *err)
{
    typedef hipcub::BlockScan<int, COD_THREADS> Scan;
    __shared__ __attribute__((aligned(16))) unsigned char stage[COD_LINE + COD_SLICE];
    __shared__ typename Scan::TempStorage scan_tmp;
    const int tid = threadIdx.x, k = k0 + blockIdx.x;
    const bcfgpu_vcf_vec v = vec[k];
    const unsigned char *run = text + v.off;
    uint32_t *st = start ? start + (size_t)blockIdx.x * ((size_t)n_smpl_in + 1) : nullptr;
    const uint4 *lines = reinterpret_cast<const uint4*>(stage);
    unsigned long long base = 0;                                            // tabs of the slices before this one
    for (unsigned long long b0 = 0; b0 < v.len; b0 += COD_SLICE) {
        const int nb = v.len - b0 < (unsigned long long)COD_SLICE ? (int)(v.len - b0) : COD_SLICE;
        const int sh = line_load(stage, run + b0, nb, tid);
        __syncthreads();
        // the lane's lines: stage bytes [q0, q0 + 64), of which [sh, sh + nb) are the slice.  Lanes read 16 bytes, 64 bytes apart:
        // how these meet on the banks is not measured
        const int q0 = tid * VDEC_LANE_LINES * COD_LINE;
        int cnt = 0;
        #pragma unroll
        for (int l = 0; l < VDEC_LANE_LINES; ++l) {
            const int q = q0 + l * COD_LINE;
            if (q < sh + nb && q + COD_LINE > sh) cnt += __popc(line_match(lines[q / COD_LINE], '\t') & bit_range(sh - q, sh + nb - q));
        }
        int at, total;
        Scan(scan_tmp).ExclusiveSum(cnt, at, total);
        if (st && cnt) {
            unsigned long long ord = base + (unsigned long long)at;
            #pragma unroll
            for (int l = 0; l < VDEC_LANE_LINES; ++l) {
                const int q = q0 + l * COD_LINE;
                if (!(q < sh + nb && q + COD_LINE > sh)) continue;
                for (uint32_t m = line_match(lines[q / COD_LINE], '\t') & bit_range(sh - q, sh + nb - q); m; m &= m - 1, ++ord)
                    if (ord < (unsigned long long)n_smpl_in) st[ord] = (uint32_t)(b0 + (unsigned long long)(q + __ffs(m) - 1 - sh));     // (a tab too many has no place)
            }
        }
        base += (unsigned long long)total;
        __syncthreads();
    }
    if (tid == 0) {
        if (st) st[n_smpl_in] = v.len;
        if (base != (unsigned long long)n_smpl_in || v.len == 0 || run[0] != '\t') atomicMin(err, (uint32_t)k);
    }
}

__global__ __launch_bounds__(COD_THREADS) void vcfdec_parse_kernel(const unsigned char *text, const bcfgpu_vcf_vec *vec, int k0, const uint32_t *start,
                                                                   const int32_t *col, int n_smpl_in, int n_smpl, int n_planes, int32_t *out, uint32_t *err)
{
    __shared__ __attribute__((aligned(16))) unsigned char stage[COD_LINE + COD_SLICE];
    const int tid = threadIdx.x, k = k0 + blockIdx.x;
    const bcfgpu_vcf_vec v = vec[k];
    const unsigned char *run = text + v.off;
    const uint32_t *st = start + (size_t)blockIdx.x * ((size_t)n_smpl_in + 1);
    const size_t S = (size_t)n_smpl;
    int32_t *o = out + (size_t)k * n_planes * S;
    bool ok = true;
    if (v.idx < 0 || col) {                                                 // no such key: '.'; a sample map: every lane its own column
        for (int s = tid; s < n_smpl; s += COD_THREADS) {
            const int c = col ? col[s] : s;
            ok &= text_sample(o + s, S, n_planes, run + st[c], (int)(st[c + 1] - st[c]), v.idx);
        }
    } else for (int s0 = 0; s0 < n_smpl; ) {
        // the round: the samples from s0 on whose text ends inside the stage (the first `fit` lanes: the ends only grow)
        const int s = s0 + tid;
        const uint32_t b0 = st[s0], b = s < n_smpl ? st[s] : 0u, e = s < n_smpl ? st[s + 1] : 0u;
        const int fit = __syncthreads_count(s < n_smpl && e - b0 <= (uint32_t)COD_SLICE);
        if (fit == 0) {                                                     // one column longer than the stage
            if (tid == 0) ok &= text_sample(o + s, S, n_planes, run + b, (int)(e - b), v.idx);
            s0 += 1;
            continue;
        }
        const int sh = line_load(stage, run + b0, (int)(st[s0 + fit] - b0), tid);
        __syncthreads();
        // Lanes read single bytes at offsets that depend on the columns before them: how these meet on the banks is not measured
        if (tid < fit) ok &= text_sample(o + s, S, n_planes, stage + sh + (b - b0), (int)(e - b), v.idx);
        __syncthreads();
        s0 += fit;
    }
    if (!ok) atomicMin(err + 1, (uint32_t)k);
}

// (kernels.h: bcfgpu_call_rewrite_vcf of vcfcallrw.hip indexes its records' columns with the same kernel)
void launch_vcfdec_index(const unsigned char *text, const bcfgpu_vcf_vec *vec, int k0, int n_sites, int n_smpl_in, uint32_t *start, uint32_t *err, hipStream_t s)
{
    hipLaunchKernelGGL(vcfdec_index_kernel, dim3(n_sites), dim3(COD_THREADS), 0, s, text, vec, k0, n_smpl_in, start, err);
}

}  // namespace bcfgpu

extern "C" int bcfgpu_call_decode_vcf(bcfgpu_ctx *ctx, int32_t n_sites, int32_t n_smpl_in, const void *d_text, uint64_t n_text_bytes,
                                      const bcfgpu_vcf_vec *vec, const int32_t *col, int32_t n_planes, int32_t *d_out)
{
    if (!ctx || n_sites < 0 || n_smpl_in < 1 || n_planes < 1 || (n_sites && (!vec || !d_out)) || (n_text_bytes && !d_text))
        return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_decode_vcf: bad arguments");
    hipStream_t st;
    if (bcfgpu_internal_device(ctx, &st, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_decode_vcf: bad context");
    const int S = bcfgpu_internal_cfg(ctx)->n_smpl;
    if (S < 1 || (!col && S > n_smpl_in)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_decode_vcf: more called samples than input samples and no sample map");
    if (col) for (int s = 0; s < S; ++s) if (col[s] < 0 || col[s] >= n_smpl_in) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_decode_vcf: a sample map entry outside the input samples");
    for (int k = 0; k < n_sites; ++k)
        if (vec[k].len > n_text_bytes || vec[k].off > n_text_bytes - vec[k].len) return bcfgpu_set_error(BCFGPU_E_RANGE, "bcfgpu_call_decode_vcf: a record's columns run past the end of the text");
    if (n_sites == 0) return 0;
    // the offsets of one site's columns, and how many sites' offsets the slot takes at once
    const size_t per = (size_t)n_smpl_in + 1, fits = BCFGPU_VCFDEC_START_BYTES / 4 / per;
    const int chunk = fits < 1 ? 1 : fits < (size_t)n_sites ? (int)fits : n_sites;
    const bool once = chunk == n_sites;
    const bcfgpu_vcf_vec *d_vec = (const bcfgpu_vcf_vec*)ws_upload(ctx, WS_COMPACT_VCFDEC_VEC, vec, (size_t)n_sites * sizeof *vec, 64, st);
    const int32_t *d_col = col ? (const int32_t*)ws_upload(ctx, WS_COMPACT_VCFDEC_COL, col, (size_t)S * 4, 64, st) : nullptr;
    uint32_t *d_start = (uint32_t*)bcfgpu_internal_ws(ctx, WS_COMPACT_VCFDEC_START, (size_t)chunk * per * 4);
    uint32_t *d_err = (uint32_t*)bcfgpu_internal_ws(ctx, WS_COMPACT_VCFDEC_ERR, 8);
    uint32_t *h_err = (uint32_t*)bcfgpu_internal_pinned(ctx, PIN_VCFDEC_ERR, 8);
    if (!d_vec || (col && !d_col) || !d_start || !d_err || !h_err) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_call_decode_vcf: workspace");
    const unsigned char *text = (const unsigned char*)d_text;
    // the indexing pass over every site before any plane is written: with the offsets when they all fit the slot, else counting only
    if (hipMemsetAsync(d_err, 0xff, 8, st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_decode_vcf: error word");
    launch_vcfdec_index(text, d_vec, 0, n_sites, n_smpl_in, once ? d_start : nullptr, d_err, st);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h_err, d_err, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_decode_vcf: indexing pass");
    if (h_err[0] != VDEC_NO_ERROR) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_decode_vcf: a record does not hold n_smpl_in sample columns, each behind a tab");
    for (int k0 = 0; k0 < n_sites; k0 += chunk) {
        const int nk = n_sites - k0 < chunk ? n_sites - k0 : chunk;
        if (!once) launch_vcfdec_index(text, d_vec, k0, nk, n_smpl_in, d_start, d_err, st);
        hipLaunchKernelGGL(vcfdec_parse_kernel, dim3(nk), dim3(COD_THREADS), 0, st, text, d_vec, k0, d_start, d_col, n_smpl_in, S, n_planes, d_out, d_err);
    }
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h_err, d_err, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_decode_vcf: parse pass");
    if (h_err[1] != VDEC_NO_ERROR) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_decode_vcf: a value of the selected field is not '.' or an integer inside int32");
    return 0;
}
