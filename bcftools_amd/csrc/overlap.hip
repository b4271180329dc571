// overlap.hip -- the mate-overlap quality tweak of the pileup engine, for all read pairs of a pool at once.
//
// `bcftools mpileup` switches it on with bam_mplp_init_overlaps() (mpileup.c:640); htslib's pileup then passes every
// second mate that overlaps its first mate through tweak_overlap_quality() (sam.c): at each reference position both
// reads cover with an aligned base, equal bases pool their qualities in the first read (capped at 200) and different
// bases keep 0.8 of the better quality; the other read's base drops to quality 0.  Which reads form a pair (proper pair,
// same contig, the first mate still buffered) is the pileup engine's bookkeeping and stays with the caller; this is the
// per-base arithmetic, one lane per pair: two cursors walk the CIGARs to their common aligned columns.
#include <hip/hip_runtime.h>
#include <vector>
#include "ctx.h"

namespace bcfgpu {

struct OverlapParams {
    int n_pairs;
    const int32_t *pair_a, *pair_b;
    DevPool D;                      // the reads; D.qual is rewritten in place
};

__global__ __launch_bounds__(64) void overlap_kernel(const OverlapParams P)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P.n_pairs) return;
    const DevPool &D = P.D;
    const int ra = P.pair_a[p], rb = P.pair_b[p];
    const uint32_t *ca = D.cig + D.r_cig_off[ra], *cb = D.cig + D.r_cig_off[rb];
    const int na = D.r_ncig[ra], nb = D.r_ncig[rb];
    const uint8_t *sa = D.seq16 + D.r_seq_off[ra], *sb = D.seq16 + D.r_seq_off[rb];
    uint8_t *qa = D.qual + D.r_seq_off[ra], *qb = D.qual + D.r_seq_off[rb];
    // the current aligned (M/=/X) block of each read: reference start x, query start y, columns left l
    int ka = 0, kb = 0, xa = D.r_pos[ra], ya = 0, la = 0, xb = D.r_pos[rb], yb = 0, lb = 0;
    for (;;) {
        while (la == 0 && ka < na) {
            const uint32_t c = ca[ka++];
            const int op = c & 0xf, l = (int)(c >> 4);
            if (op == 0 || op == 7 || op == 8) la = l;
            else if (op == 2 || op == 3) xa += l;
            else if (op == 1 || op == 4) ya += l;
        }
        while (lb == 0 && kb < nb) {
            const uint32_t c = cb[kb++];
            const int op = c & 0xf, l = (int)(c >> 4);
            if (op == 0 || op == 7 || op == 8) lb = l;
            else if (op == 2 || op == 3) xb += l;
            else if (op == 1 || op == 4) yb += l;
        }
        if (la == 0 || lb == 0) break;
        if (xa < xb) { const int d = min(xb - xa, la); xa += d; ya += d; la -= d; continue; }
        if (xb < xa) { const int d = min(xa - xb, lb); xb += d; yb += d; lb -= d; continue; }
        const int m = min(la, lb);
        for (int i = 0; i < m; ++i) {
            const int va = qa[ya + i], vb = qb[yb + i];
            int oa, ob;
            if (sa[ya + i] == sb[yb + i]) { oa = min(200, va + vb); ob = 0; }
            else if (va >= vb) { oa = (int)(0.8 * va); ob = 0; }
            else { ob = (int)(0.8 * vb); oa = 0; }
            qa[ya + i] = (uint8_t)oa; qb[yb + i] = (uint8_t)ob;
        }
        xa += m; ya += m; la -= m; xb += m; yb += m; lb -= m;
    }
}

}  // namespace bcfgpu

using namespace bcfgpu;

// The tweak on reads in HBM, queued on `stream`: the pool (bcfgpu_pool_overlap_tweak) or the uploaded view of the caller's reads
// (bcfgpu_overlap_tweak).  The pair arrays are the caller's: they are its own again once the stream has been waited for.
static int overlap_core(const char *who, bcfgpu_ctx *ctx, hipStream_t stream, const DevPool &D, int32_t n_pairs, const int32_t *pair_a,
                        const int32_t *pair_b)
{
    const int n = D.n_reads;
    {   // every read may be in one pair only (a second pair would race with the first on the read's qualities)
        std::vector<uint8_t> seen((size_t)n, 0);
        for (int p = 0; p < n_pairs; ++p) {
            const int a = pair_a[p], b = pair_b[p];
            if (a < 0 || a >= n || b < 0 || b >= n || a == b || seen[a] || seen[b])
                return bcfgpu_set_error(BCFGPU_E_ARG, who, "a read index is out of range or used twice");
            seen[a] = seen[b] = 1;
        }
    }
    if (n_pairs == 0 || D.n_bases == 0) return BCFGPU_OK;
    OverlapParams P{};
    P.n_pairs = n_pairs; P.D = D;
    P.pair_a = (const int32_t*)ws_upload(ctx, WS_POVL_PAIR_A, pair_a, (size_t)n_pairs * 4, 64, stream);
    P.pair_b = (const int32_t*)ws_upload(ctx, WS_POVL_PAIR_B, pair_b, (size_t)n_pairs * 4, 64, stream);
    if (!P.pair_a || !P.pair_b) return bcfgpu_set_error(BCFGPU_E_NOMEM, who, "device workspace or upload");
    hipLaunchKernelGGL(overlap_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, stream, P);
    if (hipGetLastError() != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, who, "launch");
    return BCFGPU_OK;
}

extern "C" int bcfgpu_overlap_tweak(bcfgpu_ctx *ctx, const bcfgpu_reads *rd, int32_t n_pairs, const int32_t *pair_a,
                                    const int32_t *pair_b, uint8_t *qual_out)
{
    const char *who = "bcfgpu_overlap_tweak";
    if (!ctx || !rd || n_pairs < 0 || (n_pairs && (!pair_a || !pair_b)) || !qual_out || rd->n_reads < 0)
        return bcfgpu_set_error(BCFGPU_E_ARG, who, "bad arguments");
    hipStream_t stream = nullptr;
    if (bcfgpu_internal_device(ctx, &stream, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, who, "bad context");
    DevPool V{};
    int rc = pool_view_upload(who, ctx, rd, nullptr, 0, POOL_VIEW, stream, &V);
    if (!rc) rc = overlap_core(who, ctx, stream, V, n_pairs, pair_a, pair_b);
    // the view's qualities, rewritten or not (no pairs, no bases: the caller's own)
    if (!rc && V.n_bases && hipMemcpyAsync(qual_out, V.qual, V.n_bases, hipMemcpyDeviceToHost, stream) != hipSuccess) rc = bcfgpu_set_error(BCFGPU_E_HIP, who, "download");
    if (hipStreamSynchronize(stream) != hipSuccess && !rc) rc = bcfgpu_set_error(BCFGPU_E_HIP, who, "hipStreamSynchronize");
    return rc;
}

// The same tweak on the pool bcfgpu_pool_upload left in HBM (after bcfgpu_pool_baq): the pairs go up, nothing comes back.
extern "C" int bcfgpu_pool_overlap_tweak(bcfgpu_ctx *ctx, int32_t n_pairs, const int32_t *pair_a, const int32_t *pair_b)
{
    const char *who = "bcfgpu_pool_overlap_tweak";
    if (!ctx || n_pairs < 0 || (n_pairs && (!pair_a || !pair_b))) return bcfgpu_set_error(BCFGPU_E_ARG, who, "bad arguments");
    hipStream_t stream = nullptr;
    if (bcfgpu_internal_device(ctx, &stream, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, who, "bad context");
    const DevPool &D = *bcfgpu_internal_pool_state(ctx);
    if (!D.valid) return bcfgpu_set_error(BCFGPU_E_ARG, who, "no read pool on this context (bcfgpu_pool_upload)");
    int rc = overlap_core(who, ctx, stream, D, n_pairs, pair_a, pair_b);
    if (hipStreamSynchronize(stream) != hipSuccess && !rc) rc = bcfgpu_set_error(BCFGPU_E_HIP, who, "hipStreamSynchronize");
    return rc;
}
