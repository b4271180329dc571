// capmapq.hip -- sam_cap_mapq(b, ref, ref_len, thres) of htslib sam.c as `mpileup -C INT` applies it to every read after
// BAQ (mpileup.c:235-239): from the mismatches of the read against the reference -- their number, the sum of their base
// qualities (each capped at 33), the aligned length and the clipped bases -- a cap on the read's mapping quality, or -1:
// the read is dropped.  One lane per read: a walk over the CIGAR and the aligned bases (integer counts), then
//     t = q - 4.343 ln( prod_{i<mm} len/(i+1) ) + clip_q/5;   t > thres: -1;   cap = (int)( sqrt((thres - max(t,0))/thres) thres + .499 )
// in double, in the reference's operation order.
//
// htslib is not part of the reference tree and no golden of the reference's tests runs `mpileup -C`: the function is
// restated from htslib's published source and checked against the oracle's restatement only (parity unpinned).
#include <hip/hip_runtime.h>
#include "ctx.h"

namespace bcfgpu {

struct CapParams {
    int thres;
    DevPool D;                                  // the reads
    const char *ref; long ref_lo, ref_hi;       // the slice of the contig the reads can touch; outside it: past the end
    int32_t *out;
};

// seq_nt16_table of htslib for the letters a reference holds (IUPAC, case-insensitive; anything else is N = 15)
__device__ __forceinline__ int cap_nt16_of(char c)
{
    switch (c) {
        case 'A': case 'a': return 1;  case 'C': case 'c': return 2;  case 'G': case 'g': return 4;  case 'T': case 't': return 8;
        case '=': return 0;
        case 'M': case 'm': return 3;  case 'R': case 'r': return 5;  case 'S': case 's': return 6;  case 'V': case 'v': return 7;
        case 'W': case 'w': return 9;  case 'Y': case 'y': return 10; case 'H': case 'h': return 11; case 'K': case 'k': return 12;
        case 'D': case 'd': return 13; case 'B': case 'b': return 14;
        case 'U': case 'u': return 8;  case '0': return 1; case '1': return 2; case '2': return 4; case '3': return 8;   /* the rest of htslib's seq_nt16_table */
        default: return 15;
    }
}

__global__ __launch_bounds__(256) void cap_mapq_kernel(const CapParams P)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    const DevPool &D = P.D;
    if (r >= D.n_reads) return;
    const uint32_t *cigar = D.cig + D.r_cig_off[r];
    const uint8_t *seq = D.seq16 + D.r_seq_off[r], *qual = D.qual + D.r_seq_off[r];
    const int ncig = D.r_ncig[r];
    const int thres = P.thres < 0 ? 40 : P.thres;
    int mm = 0, q = 0, len = 0, clip_q = 0, y = 0;
    long x = D.r_pos[r];
    auto past_end = [&](long p) { return p >= P.ref_hi || p < P.ref_lo || P.ref[p - P.ref_lo] == '\0'; };
    for (int i = 0; i < ncig; ++i) {
        const int l = (int)(cigar[i] >> 4), op = (int)(cigar[i] & 0xf);
        if (op == 0 || op == 7 || op == 8) {
            int j;
            for (j = 0; j < l; ++j) {
                const int z = y + j;
                if (past_end(x + j)) break;                                // out of bounds
                const int c1 = seq[z] & 15, c2 = cap_nt16_of(P.ref[x + j - P.ref_lo]);
                if (c2 != 15 && c1 != 15 && qual[z] >= 13) {               // not ambiguous
                    ++len;
                    if (c1 && c1 != c2 && qual[z] >= 13) { ++mm; q += qual[z] > 33 ? 33 : qual[z]; }   // mismatch
                }
            }
            if (j < l) break;
            x += l; y += l; len += l;
        } else if (op == 2) {
            int j;
            for (j = 0; j < l; ++j) if (past_end(x + j)) break;
            if (j < l) break;
            x += l;
        } else if (op == 4) {
            for (int j = 0; j < l; ++j) clip_q += qual[y + j];
            y += l;
        } else if (op == 5) clip_q += 13 * l;
        else if (op == 1) y += l;
        else if (op == 3) x += l;
    }
    double t = 1;
    for (int i = 0; i < mm; ++i) t *= (double)len / (i + 1);
    t = q - 4.343 * log(t) + clip_q / 5.;
    int res;
    if (t > thres) res = -1;
    else {
        if (t < 0) t = 0;
        t = sqrt((thres - t) / thres) * thres;
        res = (int)(t + .499);
    }
    P.out[r] = res;
}

}  // namespace bcfgpu

using namespace bcfgpu;

namespace bcfgpu {
// mpileup.c:238: a read whose mapping quality is above its cap is lowered to it
__global__ __launch_bounds__(256) void cap_apply_kernel(int n, const int32_t *cap, uint8_t *mapq)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < n && cap[r] >= 0 && (int)mapq[r] > cap[r]) mapq[r] = (uint8_t)cap[r];
}
}

// sam_cap_mapq on reads in HBM, the pool (bcfgpu_pool_cap_mapq) or the uploaded view of the caller's reads (bcfgpu_cap_mapq): the
// caps come back to `cap` (HOST); apply: the reads' mapping qualities (D.r_mapq) are lowered to them in place.
static int cap_core(const char *who, bcfgpu_ctx *ctx, hipStream_t st, DevPool &D, const char *ref, int32_t ref_len, int32_t thres, int32_t *cap, bool apply)
{
    const int n = D.n_reads;
    if (!n) return BCFGPU_OK;
    int lo = 0, hi = 0;
    if (bcfgpu_internal_pool_extent(ctx, D, &lo, &hi)) return bcfgpu_set_error(BCFGPU_E_HIP, who, "pool extent");
    if (lo < 0) lo = 0;
    if (hi > ref_len) hi = ref_len;
    if (hi < lo) hi = lo;
    CapParams P{};
    P.thres = thres; P.D = D;
    char *d_ref = (char*)ws_upload(ctx, WS_PCAPQ_REF, ref + lo, (size_t)(hi - lo), 64, st);
    P.out = (int32_t*)bcfgpu_internal_ws(ctx, WS_PCAPQ_OUT, (size_t)n * 4 + 64);
    if (!d_ref || !P.out) return bcfgpu_set_error(BCFGPU_E_NOMEM, who, "device workspace or upload");
    P.ref = d_ref; P.ref_lo = lo; P.ref_hi = hi;
    hipLaunchKernelGGL(cap_mapq_kernel, dim3((n + 255) / 256), dim3(256), 0, st, P);
    if (apply) hipLaunchKernelGGL(cap_apply_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, (const int32_t*)P.out, D.r_mapq);
    if (hipGetLastError() != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, who, "launch");
    if (hipMemcpyAsync(cap, P.out, (size_t)n * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return bcfgpu_set_error(BCFGPU_E_HIP, who, "download");
    return BCFGPU_OK;
}

// On the pool in HBM (after bcfgpu_pool_baq): the caps come back for the caller's filters (cap < 0: the read is dropped,
// mpileup.c:237), the pool's mapping qualities are lowered in place.
extern "C" int bcfgpu_pool_cap_mapq(bcfgpu_ctx *ctx, const char *ref, int32_t ref_len, int32_t thres, int32_t *cap)
{
    const char *who = "bcfgpu_pool_cap_mapq";
    if (!ctx || !cap || (ref_len > 0 && !ref)) return bcfgpu_set_error(BCFGPU_E_ARG, who, "bad arguments");
    hipStream_t st = nullptr;
    if (bcfgpu_internal_device(ctx, &st, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, who, "bad context");
    DevPool &D = *bcfgpu_internal_pool_state(ctx);
    if (!D.valid) return bcfgpu_set_error(BCFGPU_E_ARG, who, "no read pool on this context (bcfgpu_pool_upload)");
    return cap_core(who, ctx, st, D, ref, ref_len, thres, cap, true);
}

// On the caller's reads: the caps only (the caller lowers its mapping qualities itself).
extern "C" int bcfgpu_cap_mapq(bcfgpu_ctx *ctx, const bcfgpu_reads *rd, const char *ref, int32_t ref_len, int32_t thres, int32_t *cap)
{
    const char *who = "bcfgpu_cap_mapq";
    if (!ctx || !rd || !cap || rd->n_reads < 0 || (ref_len > 0 && !ref)) return bcfgpu_set_error(BCFGPU_E_ARG, who, "bad arguments");
    hipStream_t st = nullptr;
    if (bcfgpu_internal_device(ctx, &st, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, who, "bad context");
    if (!rd->n_reads) return BCFGPU_OK;
    DevPool V{};
    int rc = pool_view_upload(who, ctx, rd, nullptr, 0, POOL_VIEW, st, &V);
    if (!rc) rc = cap_core(who, ctx, st, V, ref, ref_len, thres, cap, false);
    if (rc) hipStreamSynchronize(st);                           // (the copies read the caller's arrays)
    return rc;
}
