// calsmap.hip -- `call -C alleles`: the PL and AD / QS planes of records re-expressed in the alleles of their targets, made on the
// device from the planes bcfgpu_call_decode_bcf / _vcf left in HBM: the per-sample part of mcall_constrain_alleles (mcall.c:1332-1371
// the PL gather through pl_map with the unseen allele standing in, :1380-1413 the Number=R tags through als_map), as
// host/bcfgpu_call.c constrain_line() prints it and build_planes() parses it back.
//
//   cals_kernel<MODE>  one wavefront a (site, 64 samples): lanes run along samples, so every plane read and every plane store of a
//                      wavefront is 64 consecutive int32.  The site's descriptor is wavefront-uniform (the site index goes through
//                      readfirstlane): it is loaded into scalar registers, and amap / pl_map are formed from it with compile-time
//                      (i, j) -- a fold over the 15 genotypes, no array, no run-time index.  The plane of a genotype is a scalar
//                      offset, its load one global_load_dword a lane.  The fallback for a `missing` value (the alleles mpileup did
//                      not see) is the per-lane branch and loads only there.  Sites of any shape share the grid: the wavefronts
//                      stride over the (site, chunk) pairs.
#include <utility>
#include "ctx.h"

using namespace bcfgpu;

static_assert(sizeof(bcfgpu_cals_site) == 32, "bcfgpu_cals_site is 32 bytes");
static_assert(BCFGPU_MAX_ALLELES == 5, "cals_kernel unrolls over 5 alleles, 15 genotypes");

namespace bcfgpu {

constexpr int CALS_THREADS = 256, CALS_WAVE = 64;
constexpr unsigned CALS_AL_CAP = 0xFFFFu;     // an allele index counts as at most this: gt() stays inside 32 bits, and past every n_in

__device__ __forceinline__ unsigned cals_gt(unsigned a, unsigned b) { return a > b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; }
__device__ __forceinline__ unsigned cals_cap(int32_t a) { return (unsigned)a < CALS_AL_CAP ? (unsigned)a : CALS_AL_CAP; }
template <int I> __device__ __forceinline__ unsigned cals_amap(const bcfgpu_cals_site &d) { return cals_cap(d.amap[I]); }

// plane m of the lane's sample, `end of vector` past the input's planes (m is wavefront-uniform where the caller's is)
__device__ __forceinline__ int32_t cals_in(const int32_t *pin, size_t S, unsigned n_in, unsigned m)
{
    return m < n_in ? pin[(size_t)m * S] : BCFGPU_INT32_VECTOR_END;
}

struct CalsLane { const int32_t *pin; int32_t *po; size_t S; unsigned n_in; bool ended; };

// genotype G of the constrained record (mcall.c:1332-1371)
template <int G> __device__ __forceinline__ void cals_pl_cell(const bcfgpu_cals_site &d, int ng, CalsLane &L)
{
    constexpr int I = G < 1 ? 0 : G < 3 ? 1 : G < 6 ? 2 : G < 10 ? 3 : 4, J = G - I * (I + 1) / 2;
    if (G >= ng) return;                                                // (uniform)
    const unsigned a = cals_amap<I>(d), b = cals_amap<J>(d), lo = a < b ? a : b, hi = a < b ? b : a;
    int32_t v = cals_in(L.pin, L.S, L.n_in, hi * (hi + 1) / 2 + lo);
    if (v == BCFGPU_INT32_MISSING && d.unseen >= 0) {                   // an allele mpileup did not see: the unseen allele stands in
        const unsigned u = cals_cap(d.unseen);
        int32_t x = cals_in(L.pin, L.S, L.n_in, cals_gt(lo, u));
        if (x == BCFGPU_INT32_MISSING) x = cals_in(L.pin, L.S, L.n_in, cals_gt(hi, u));
        if (x == BCFGPU_INT32_MISSING) x = cals_in(L.pin, L.S, L.n_in, cals_gt(u, u));
        v = x;
    }
    if (G == 0 && v == BCFGPU_INT32_VECTOR_END) v = BCFGPU_INT32_MISSING;
    L.ended |= v == BCFGPU_INT32_VECTOR_END;                            // the text is cut here and parsed back
    L.po[(size_t)G * L.S] = L.ended ? BCFGPU_INT32_VECTOR_END : v;
}
template <int... Gs> __device__ __forceinline__ void cals_pl_cells(const bcfgpu_cals_site &d, int ng, CalsLane &L, std::integer_sequence<int, Gs...>)
{
    (cals_pl_cell<Gs>(d, ng, L), ...);
}

// allele A of a Number=R vector (mcall.c:1380-1413): nv = the sample's values, dot = its vector is the one value `missing`
template <int A> __device__ __forceinline__ void cals_r_cell(const bcfgpu_cals_site &d, CalsLane &L, unsigned nv, bool dot)
{
    if (A >= d.n_new) return;                                           // (uniform)
    const unsigned m = cals_amap<A>(d);
    const int32_t x = cals_in(L.pin, L.S, L.n_in, m);
    int32_t v = m < nv ? x : BCFGPU_INT32_MISSING;
    if (dot) v = A == 0 ? BCFGPU_INT32_MISSING : BCFGPU_INT32_VECTOR_END;
    L.po[(size_t)A * L.S] = v;
}
template <int... As> __device__ __forceinline__ void cals_r_cells(const bcfgpu_cals_site &d, CalsLane &L, unsigned nv, bool dot, std::integer_sequence<int, As...>)
{
    (cals_r_cell<As>(d, L, nv, dot), ...);
}

template <int MODE>
__global__ __launch_bounds__(CALS_THREADS) void cals_kernel(const bcfgpu_cals_site *site, long long n_work, int chunks, int n_smpl,
                                                            int n_in, const int32_t *in, int n_out, int32_t *out)
{
    const int lane = threadIdx.x & (CALS_WAVE - 1);
    const long long w0 = (long long)blockIdx.x * (CALS_THREADS / CALS_WAVE) + threadIdx.x / CALS_WAVE, dw = (long long)gridDim.x * (CALS_THREADS / CALS_WAVE);
    const size_t S = (size_t)n_smpl;
    for (long long w = w0; w < n_work; w += dw) {
        const int k = __builtin_amdgcn_readfirstlane((int)(w / chunks)), c = __builtin_amdgcn_readfirstlane((int)(w % chunks));
        const int s = c * CALS_WAVE + lane;
        if (s >= n_smpl) continue;
        const bcfgpu_cals_site d = site[k];
        CalsLane L = { in + (size_t)k * n_in * S + s, out + (size_t)k * n_out * S + s, S, (unsigned)n_in, false };
        if (!d.changed) {                                               // the line as it is
            for (int g = 0; g < n_out; ++g) L.po[(size_t)g * S] = cals_in(L.pin, S, L.n_in, (unsigned)g);
            continue;
        }
        int n_set;
        if (MODE == 0) {
            n_set = d.n_new * (d.n_new + 1) / 2;
            cals_pl_cells(d, n_set, L, std::make_integer_sequence<int, 15>{});
        } else {
            unsigned nv = 0; bool open = true; int32_t first = BCFGPU_INT32_VECTOR_END;
            for (int j = 0; j < n_in; ++j) {
                const int32_t x = L.pin[(size_t)j * S];
                if (j == 0) first = x;
                open = open && x != BCFGPU_INT32_VECTOR_END;
                nv += open;
            }
            n_set = d.n_new;
            cals_r_cells(d, L, nv, nv == 1 && first == BCFGPU_INT32_MISSING, std::make_integer_sequence<int, 5>{});
        }
        for (int g = n_set; g < n_out; ++g) L.po[(size_t)g * S] = BCFGPU_INT32_VECTOR_END;
    }
}

}  // namespace bcfgpu

extern "C" int bcfgpu_call_constrain(bcfgpu_ctx *ctx, int32_t mode, int32_t n_sites, const bcfgpu_cals_site *site,
                                     int32_t n_in, const int32_t *d_in, int32_t n_out, int32_t *d_out)
{
    if (!ctx || n_sites < 0 || n_in < 1 || n_out < 1 || n_in > BCFGPU_CALS_MAX_PLANES || n_out > BCFGPU_CALS_MAX_PLANES || (n_sites && (!site || !d_in || !d_out)))
        return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_constrain: bad arguments");
    if (mode != BCFGPU_CALS_NUMBER_G && mode != BCFGPU_CALS_NUMBER_R) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_constrain: unknown mode");
    hipStream_t st;
    if (bcfgpu_internal_device(ctx, &st, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_constrain: bad context");
    const int S = bcfgpu_internal_cfg(ctx)->n_smpl;
    if (S < 1) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_constrain: no samples");
    for (int k = 0; k < n_sites; ++k) {
        const bcfgpu_cals_site *d = &site[k];
        if (d->n_new < 1 || d->n_new > BCFGPU_MAX_ALLELES) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_constrain: a site's n_new is not 1-5");
        for (int i = 0; i < d->n_new; ++i) if (d->amap[i] < 0) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_constrain: a negative amap entry");
        const int need = mode == BCFGPU_CALS_NUMBER_G ? d->n_new * (d->n_new + 1) / 2 : d->n_new;
        if (d->changed && need > n_out) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_constrain: a changed site's vector does not fit n_out");
    }
    if (n_sites == 0) return 0;
    {
        const uintptr_t i0 = (uintptr_t)d_in, o0 = (uintptr_t)d_out;
        const uint64_t li = (uint64_t)n_sites * (uint64_t)n_in * (uint64_t)S * 4, lo = (uint64_t)n_sites * (uint64_t)n_out * (uint64_t)S * 4;
        if (i0 < o0 + lo && o0 < i0 + li) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_constrain: d_out overlaps d_in");
    }
    const bcfgpu_cals_site *d_site = (const bcfgpu_cals_site*)ws_upload(ctx, WS_COMPACT_CALS_SITE, site, (size_t)n_sites * sizeof *site, 64, st);
    if (!d_site) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_call_constrain: workspace");
    const int chunks = (S + CALS_WAVE - 1) / CALS_WAVE, per_block = CALS_THREADS / CALS_WAVE;
    const long long n_work = (long long)n_sites * chunks, want = (n_work + per_block - 1) / per_block;
    const unsigned blocks = (unsigned)(want < (1ll << 20) ? want : (1ll << 20));      // the wavefronts stride over the rest
    if (mode == BCFGPU_CALS_NUMBER_G) hipLaunchKernelGGL(cals_kernel<0>, dim3(blocks), dim3(CALS_THREADS), 0, st, d_site, n_work, chunks, S, n_in, d_in, n_out, d_out);
    else hipLaunchKernelGGL(cals_kernel<1>, dim3(blocks), dim3(CALS_THREADS), 0, st, d_site, n_work, chunks, S, n_in, d_in, n_out, d_out);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_constrain: constrain pass");
    return 0;
}
