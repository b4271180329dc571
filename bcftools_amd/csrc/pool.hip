// pool.hip -- the read pool of a region in HBM: the caller's reads (a bcfgpu_reads, or the packed forms of bcfgpu_packed) brought
// up once, as the one-byte-per-base arrays every read stage indexes (baq.hip, overlap.hip, capmapq.hip, gap_prep.hip) and the
// pileup is built from (pileup.hip).
//
// Defined here: the uploaded view of a bcfgpu_reads (pool_view_upload), the two halves of an upload (pool_copy: the host-to-device
// copies; pool_form: the kernels that expand the packed forms) with the entry points made of them -- bcfgpu_pool_upload, and
// bcfgpu_pool_stage + bcfgpu_pool_adopt, the same upload cut in two around a copy stream --, bcfgpu_pool_keep,
// bcfgpu_pool_download and the pool's extent on the reference (bcfgpu_internal_pool_extent).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "ctx.h"

namespace bcfgpu {

// [lowest start, highest end) of the pool's reads on the reference
__global__ __launch_bounds__(256) void pool_extent_kernel(const DevPool D, int *out)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    int lo = INT32_MAX, hi = 0;
    if (r < D.n_reads) {
        int x = D.r_pos[r];
        lo = x;
        const uint32_t *cg = D.cig + D.r_cig_off[r];
        for (int k = 0; k < D.r_ncig[r]; ++k) { const int op = cg[k] & 15; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) x += (int)(cg[k] >> 4); }
        hi = x;
    }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
    if ((threadIdx.x & 63) == 0 && lo != INT32_MAX) { atomicMin(&out[0], lo); atomicMax(&out[1], hi); }
}

// bcfgpu_read12 records to the per-read arrays the stages index; the lengths (rounded up to four bases) and operation counts
// in the offset arrays, which an exclusive prefix sum then turns into r_seq_off / r_cig_off
__global__ __launch_bounds__(256) void pool_expand_kernel(const bcfgpu_read12 *rec, int n, int32_t *r_pos, int32_t *r_lq, int32_t *r_flag,
                                                         int32_t *r_ncig, int32_t *r_cig_off, int32_t *r_seq_off, uint8_t *r_mapq)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r > n) return;
    if (r == n) { r_cig_off[n] = 0; r_seq_off[n] = 0; return; }           // (the scans run over n + 1 elements)
    const uint32_t *w = reinterpret_cast<const uint32_t*>(rec + r);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    const int lq = (int)(w1 & 0xffff), ncig = (int)((w1 >> 16) & 0xff), f8 = (int)(w1 >> 24);
    r_pos[r] = (int32_t)w0; r_lq[r] = lq; r_ncig[r] = ncig; r_flag[r] = ((f8 & 1) ? 16 : 0) | ((f8 & 2) ? 4 : 0);
    r_mapq[r] = (uint8_t)(w2 & 0xff);
    r_seq_off[r] = (lq + 3) & ~3; r_cig_off[r] = ncig;
}

// The pool as BAM records hold it (two 4-bit base codes per byte, high nibble first) and qualities as palette indices, to the
// one-byte-per-base arrays every kernel of the host-fed stages reads.  A lane per four input bytes = eight bases.
__global__ __launch_bounds__(256) void pileup_unpack_kernel(const uint8_t *seq4, const uint8_t *qual4, unsigned long long pal_lo,
                                                            unsigned long long pal_hi, size_t n_in, uint8_t *seq16, uint8_t *qual, int qual_bits)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (4 * t >= n_in) return;
    if (qual4 && qual_bits == 2) {               // four indices per byte: this lane's eight bases are two input bytes
        const uint32_t v = *reinterpret_cast<const uint16_t*>(qual4 + 2 * t);
        uint32_t lo = 0, hi = 0;
        #pragma unroll
        for (int b = 0; b < 4; ++b) {
            lo |= (uint32_t)((pal_lo >> (8 * ((v >> (6 - 2 * b)) & 3))) & 0xff) << (8 * b);
            hi |= (uint32_t)((pal_lo >> (8 * ((v >> (14 - 2 * b)) & 3))) & 0xff) << (8 * b);
        }
        *reinterpret_cast<uint2*>(qual + 8 * t) = make_uint2(lo, hi);
        qual4 = nullptr;
    }
    if (seq4) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(seq4 + 4 * t);
        uint32_t lo = 0, hi = 0;
        #pragma unroll
        for (int b = 0; b < 2; ++b) {
            const uint32_t by = (v >> (8 * b)) & 0xff, by2 = (v >> (8 * b + 16)) & 0xff;
            lo |= ((by >> 4) | (by & 15) << 8) << (16 * b);
            hi |= ((by2 >> 4) | (by2 & 15) << 8) << (16 * b);
        }
        *reinterpret_cast<uint2*>(seq16 + 8 * t) = make_uint2(lo, hi);
    }
    if (qual4) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(qual4 + 4 * t);
        auto pal = [&](uint32_t j) -> uint32_t { return (uint32_t)(((j & 8) ? pal_hi : pal_lo) >> (8 * (j & 7))) & 0xff; };
        uint32_t lo = 0, hi = 0;
        #pragma unroll
        for (int b = 0; b < 2; ++b) {
            const uint32_t by = (v >> (8 * b)) & 0xff, by2 = (v >> (8 * b + 16)) & 0xff;
            lo |= (pal(by >> 4) | pal(by & 15) << 8) << (16 * b);
            hi |= (pal(by2 >> 4) | pal(by2 & 15) << 8) << (16 * b);
        }
        *reinterpret_cast<uint2*>(qual + 8 * t) = make_uint2(lo, hi);
    }
}

}  // namespace bcfgpu

using namespace bcfgpu;

// ---- the read pool in HBM ---------------------------------------------------------------------------------------------
// The host part is argument checks, uploads of the caller's arrays as they are, and launches.

int bcfgpu::host_threads(int n)
{
    int nthr = (int)std::thread::hardware_concurrency();
    if (const char *e = getenv("BCFGPU_HOST_THREADS")) nthr = atoi(e);
    return std::max(1, std::min(std::min(nthr, 16), n / 262144 + 1));
}

// The pool's kept slots come in two sets (ctx.h): the context's pool lies in one, the pool bcfgpu_pool_stage brings up in the other.
// (zq / r_has_zq: no upload writes them; bcfgpu_pool_baq leaves the pool's there, whichever set it is in)
static const PoolSlots POOL_SET[2] = {
    {WS_POOL_CIG, WS_POOL_SEQ16, WS_POOL_QUAL, WS_POOL_R_POS, WS_POOL_R_LQ, WS_POOL_R_FLAG, WS_POOL_R_NCIG, WS_POOL_R_CIG_OFF, WS_POOL_R_SEQ_OFF, WS_POOL_R_MAPQ,
     WS_PBAQ_ZQ, WS_PBAQ_HAS_ZQ},
    {WS_POOL_B_CIG, WS_POOL_B_SEQ16, WS_POOL_B_QUAL, WS_POOL_B_R_POS, WS_POOL_B_R_LQ, WS_POOL_B_R_FLAG, WS_POOL_B_R_NCIG, WS_POOL_B_R_CIG_OFF, WS_POOL_B_R_SEQ_OFF,
     WS_POOL_B_R_MAPQ, WS_PBAQ_ZQ, WS_PBAQ_HAS_ZQ},
};
// where the packed inputs go: scratch of one call (bcfgpu_pool_upload), or kept from the stage to the adopt
struct PackedSlots { WsSlot seq4, qual4, recs; };
static const PackedSlots PACKED_SCRATCH = {WS_POOL_SEQ4, WS_POOL_QUAL4, WS_POOL_RECS}, PACKED_STAGED = {WS_POOL_STAGE_SEQ4, WS_POOL_STAGE_QUAL4, WS_POOL_STAGE_RECS};

static int pool_fail(const char *who, int code, const char *what)
{
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return bcfgpu_set_error(code, msg);
}

static int pool_check_args(const char *who, bcfgpu_ctx *ctx, const bcfgpu_reads *rd, const bcfgpu_packed *pk, const uint8_t *r_mapq)
{
    const bool recs = pk && pk->recs;
    if (!ctx || !rd || rd->n_reads < 0 || (rd->n_reads && !recs && !r_mapq)) return pool_fail(who, BCFGPU_E_ARG, "bad arguments");
    if (rd->n_reads && ((!recs && (!rd->r_pos || !rd->r_lq || !rd->r_flag || !rd->r_ncig || !rd->r_cig_off || !rd->r_seq_off)) ||
                        (!pk && !rd->seq16) || (!(pk && pk->qual4) && !rd->qual)))
        return pool_fail(who, BCFGPU_E_ARG, "a read array is missing");
    if (pk && (!pk->seq4 || pk->n_bases < 0 || pk->n_cig < 0 || (pk->n_bases >> 32) || (pk->qual_bits != 0 && pk->qual_bits != 2 && pk->qual_bits != 4)))
        return pool_fail(who, BCFGPU_E_ARG, "bad packed pool");
    return BCFGPU_OK;
}

// the per-read arrays of `rd` as they are (pool_view_upload, and the packed form that brings its own bases only)
static void upload_read_arrays(bcfgpu_ctx *ctx, const bcfgpu_reads *rd, const uint8_t *r_mapq, unsigned want, const PoolSlots &ps, hipStream_t stream, DevPool &D)
{
    const size_t n = (size_t)rd->n_reads;
    D.r_pos = (const int32_t*)ws_upload(ctx, ps.r_pos, rd->r_pos, n * 4, 64, stream);
    D.r_lq = (want & READS_LQ) ? (const int32_t*)ws_upload(ctx, ps.r_lq, rd->r_lq, n * 4, 64, stream) : nullptr;
    D.r_flag = (want & READS_FLAG) ? (const int32_t*)ws_upload(ctx, ps.r_flag, rd->r_flag, n * 4, 64, stream) : nullptr;
    D.r_ncig = (const int32_t*)ws_upload(ctx, ps.r_ncig, rd->r_ncig, n * 4, 64, stream);
    D.r_cig_off = (const int32_t*)ws_upload(ctx, ps.r_cig_off, rd->r_cig_off, n * 4, 64, stream);
    D.r_seq_off = (const int32_t*)ws_upload(ctx, ps.r_seq_off, rd->r_seq_off, n * 4, 64, stream);
    D.r_mapq = (want & READS_MAPQ) ? (uint8_t*)ws_upload(ctx, ps.r_mapq, r_mapq, n, 64, stream) : nullptr;
}

int bcfgpu::pool_view_upload(const char *who, bcfgpu_ctx *ctx, const bcfgpu_reads *rd, const uint8_t *r_mapq, unsigned want,
                             const PoolSlots &ps, hipStream_t stream, DevPool *out)
{
    const int n = rd->n_reads;
    if (n && (!rd->r_pos || !rd->r_lq || !rd->r_ncig || !rd->r_cig_off || !rd->r_seq_off || !rd->seq16 || !rd->qual ||
              ((want & READS_FLAG) && !rd->r_flag) || ((want & READS_MAPQ) && !r_mapq)))
        return pool_fail(who, BCFGPU_E_ARG, "a read array is missing");
    const int nthr = host_threads(n);
    std::vector<size_t> t_nbase(nthr, 0), t_ncig(nthr, 0);
    on_threads(nthr, [&](int t) {
        const int k0 = (int)((long)n * t / nthr), k1 = (int)((long)n * (t + 1) / nthr);
        size_t nb = 0, nc = 0;
        for (int r = k0; r < k1; ++r) {
            const size_t e = (size_t)rd->r_seq_off[r] + (size_t)std::max(rd->r_lq[r], 0), c = (size_t)rd->r_cig_off[r] + (size_t)std::max(rd->r_ncig[r], 0);
            if (e > nb) nb = e;
            if (c > nc) nc = c;
        }
        t_nbase[t] = nb; t_ncig[t] = nc;
    });
    size_t nbase = 0, ncig = 0;
    for (int t = 0; t < nthr; ++t) { nbase = std::max(nbase, t_nbase[t]); ncig = std::max(ncig, t_ncig[t]); }
    if (nbase >> 32) return pool_fail(who, BCFGPU_E_RANGE, "the pool holds 2^32 or more bases");
    DevPool D{};
    D.n_reads = n; D.n_bases = (uint32_t)nbase; D.n_cig = (uint32_t)ncig;
    upload_read_arrays(ctx, rd, r_mapq, want, ps, stream, D);
    D.cig = (const uint32_t*)ws_upload(ctx, ps.cig, rd->cig, ncig * 4, 64, stream);
    D.seq16 = (const uint8_t*)ws_upload(ctx, ps.seq16, rd->seq16, nbase, 64, stream);
    D.qual = (uint8_t*)ws_upload(ctx, ps.qual, rd->qual, nbase, 64, stream);
    D.qual_slot = ps.qual;
    const bool zq = (want & READS_ZQ) && rd->zq && rd->r_has_zq;
    if (zq) {
        D.zq = (uint8_t*)ws_upload(ctx, ps.zq, rd->zq, nbase, 64, stream);
        D.r_has_zq = (uint8_t*)ws_upload(ctx, ps.r_has_zq, rd->r_has_zq, (size_t)n, 64, stream);
    }
    if (!D.r_pos || ((want & READS_LQ) && !D.r_lq) || ((want & READS_FLAG) && !D.r_flag) || !D.r_ncig || !D.r_cig_off || !D.r_seq_off || ((want & READS_MAPQ) && !D.r_mapq) ||
        !D.cig || !D.seq16 || !D.qual || (zq && (!D.zq || !D.r_has_zq)))
        return pool_fail(who, BCFGPU_E_NOMEM, "device workspace");
    *out = D;
    return BCFGPU_OK;
}

// The caller's arrays to HBM: every host-to-device copy of a pool, queued on `stream`, into set `ps` of the pool's slots and (the
// packed inputs) into `pks`.  `in` becomes the pool's description: D's arrays all have their room, those of the packed forms are
// formed by pool_form.  No kernel is launched here.
static int pool_copy(const char *who, bcfgpu_ctx *ctx, const bcfgpu_reads *rd, const bcfgpu_packed *pk, const uint8_t *r_mapq,
                     const PoolSlots &ps, const PackedSlots &pks, hipStream_t stream, PoolStage &in)
{
    auto fail = [&](int code, const char *what) { return pool_fail(who, code, what); };
    in.d_rec = nullptr; in.d_seq4 = in.d_qual4 = nullptr; in.qual_bits = 0; in.pal[0] = in.pal[1] = 0;
    if (!pk) return pool_view_upload(who, ctx, rd, r_mapq, READS_LQ | READS_FLAG | READS_MAPQ, ps, stream, &in.D);
    // the packed forms state the extent of the pools
    DevPool D{};
    const int n = rd->n_reads;
    const size_t nbase = (size_t)pk->n_bases, ncig = (size_t)pk->n_cig;
    D.n_reads = n; D.n_bases = (uint32_t)nbase; D.n_cig = (uint32_t)ncig;
    if (pk->recs) {
        // the 12-byte records: the arrays are formed from them, the offsets by two prefix sums (pool_form)
        in.d_rec = (const bcfgpu_read12*)ws_upload(ctx, pks.recs, pk->recs, (size_t)n * sizeof(bcfgpu_read12), 64, stream);
        D.r_pos = (const int32_t*)bcfgpu_internal_ws(ctx, ps.r_pos, (size_t)n * 4 + 64); D.r_lq = (const int32_t*)bcfgpu_internal_ws(ctx, ps.r_lq, (size_t)n * 4 + 64);
        D.r_flag = (const int32_t*)bcfgpu_internal_ws(ctx, ps.r_flag, (size_t)n * 4 + 64); D.r_ncig = (const int32_t*)bcfgpu_internal_ws(ctx, ps.r_ncig, (size_t)n * 4 + 64);
        D.r_cig_off = (const int32_t*)bcfgpu_internal_ws(ctx, ps.r_cig_off, (size_t)(n + 1) * 4 + 64); D.r_seq_off = (const int32_t*)bcfgpu_internal_ws(ctx, ps.r_seq_off, (size_t)(n + 1) * 4 + 64);
        D.r_mapq = (uint8_t*)bcfgpu_internal_ws(ctx, ps.r_mapq, (size_t)n + 64);
        if (!in.d_rec) return fail(BCFGPU_E_NOMEM, "device workspace");
    } else upload_read_arrays(ctx, rd, r_mapq, READS_LQ | READS_FLAG | READS_MAPQ, ps, stream, D);
    D.cig = (const uint32_t*)ws_upload(ctx, ps.cig, rd->cig, ncig * 4, 64, stream);
    const size_t n_in = (nbase + 1) / 2;
    D.seq16 = (const uint8_t*)bcfgpu_internal_ws(ctx, ps.seq16, nbase + 64);
    in.d_seq4 = (const uint8_t*)ws_upload(ctx, pks.seq4, pk->seq4, n_in, 64, stream);
    if (pk->qual4) {
        D.qual = (uint8_t*)bcfgpu_internal_ws(ctx, ps.qual, nbase + 64);
        in.d_qual4 = (const uint8_t*)ws_upload(ctx, pks.qual4, pk->qual4, pk->qual_bits == 2 ? (nbase + 3) / 4 : n_in, 64, stream);
    } else D.qual = (uint8_t*)ws_upload(ctx, ps.qual, rd->qual, nbase, 64, stream);
    D.qual_slot = ps.qual;
    std::memcpy(in.pal, pk->palette, 16);
    in.qual_bits = (int)pk->qual_bits;
    if (!in.d_seq4 || (pk->qual4 && !in.d_qual4) || !D.r_pos || !D.r_lq || !D.r_flag || !D.r_ncig || !D.r_cig_off || !D.r_seq_off || !D.r_mapq ||
        !D.cig || !D.seq16 || !D.qual)
        return fail(BCFGPU_E_NOMEM, "device workspace");
    in.D = D;
    return BCFGPU_OK;
}

// The pool pool_copy described, formed on `stream` (behind its copies) and made the context's read pool: the packed forms are
// expanded to the arrays the stages index; the plain form's arrays are already what the caller handed over.
static int pool_form(const char *who, bcfgpu_ctx *ctx, const PoolStage &in, hipStream_t stream)
{
    auto fail = [&](int code, const char *what) { return pool_fail(who, code, what); };
    const DevPool &S = in.D;
    const int n = S.n_reads;
    if (in.d_rec) {
        int32_t *a_coff = const_cast<int32_t*>(S.r_cig_off), *a_soff = const_cast<int32_t*>(S.r_seq_off);
        hipLaunchKernelGGL(pool_expand_kernel, dim3((n + 256) / 256), dim3(256), 0, stream, in.d_rec, n, const_cast<int32_t*>(S.r_pos), const_cast<int32_t*>(S.r_lq),
                           const_cast<int32_t*>(S.r_flag), const_cast<int32_t*>(S.r_ncig), a_coff, a_soff, S.r_mapq);
        int rc = scan_exclusive(ctx, stream, WS_POOL_SCAN_TMP, a_soff, n + 1);
        if (!rc) rc = scan_exclusive(ctx, stream, WS_POOL_SCAN_TMP, a_coff, n + 1);
        if (rc) return fail(rc, rc == BCFGPU_E_HIP ? "scan" : "device workspace");
    }
    if (in.d_seq4) {
        const size_t n_in = ((size_t)S.n_bases + 1) / 2, nthreads = (n_in + 3) / 4;
        if (nthreads) hipLaunchKernelGGL(pileup_unpack_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, stream,
                                         in.d_seq4, in.d_qual4, in.pal[0], in.pal[1], n_in, const_cast<uint8_t*>(S.seq16), S.qual, in.qual_bits);
    }
    if (hipGetLastError() != hipSuccess) return fail(BCFGPU_E_HIP, "launch");
    DevPool &D = *bcfgpu_internal_pool_state(ctx);
    D = S;
    D.valid = 1;
    return BCFGPU_OK;
}

int bcfgpu::pool_upload_impl(const char *who, bcfgpu_ctx *ctx, const bcfgpu_reads *rd, const bcfgpu_packed *pk, const uint8_t *r_mapq)
{
    if (const int rc = pool_check_args(who, ctx, rd, pk, r_mapq)) return rc;
    hipStream_t stream = nullptr;
    if (bcfgpu_internal_device(ctx, &stream, nullptr)) return pool_fail(who, BCFGPU_E_ARG, "bad context");
    bcfgpu_internal_pool_replaced(ctx);
    // into the set the context's pool is in (a staged pool, in the other one, stays as it is), everything on the context's stream
    PoolStage in;
    const int rc = pool_copy(who, ctx, rd, pk, r_mapq, POOL_SET[bcfgpu_internal_pool_stage(ctx, false)->set], PACKED_SCRATCH, stream, in);
    return rc ? rc : pool_form(who, ctx, in, stream);
}

// ---- the pool as an object of its own: upload once, run the stages on it, build the tile ----
// [lowest start, highest end) of D's reads (one small kernel and a wait, once per pool)
int bcfgpu::bcfgpu_internal_pool_extent(bcfgpu_ctx *ctx, DevPool &D, int *lo, int *hi)
{
    hipStream_t stream = nullptr;
    if (bcfgpu_internal_device(ctx, &stream, nullptr)) return BCFGPU_E_ARG;
    if (!D.ext_valid) {
        int *d = (int*)bcfgpu_internal_ws(ctx, WS_POOL_EXTENT, 64);
        if (!d) return BCFGPU_E_NOMEM;
        int v[2] = {INT32_MAX, 0};
        if (hipMemcpyAsync(d, v, 8, hipMemcpyHostToDevice, stream) != hipSuccess) return BCFGPU_E_HIP;
        if (D.n_reads) hipLaunchKernelGGL(pool_extent_kernel, dim3((D.n_reads + 255) / 256), dim3(256), 0, stream, D, d);
        if (hipMemcpyAsync(v, d, 8, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return BCFGPU_E_HIP;
        if (v[0] == INT32_MAX) v[0] = 0;
        D.ext_lo = v[0]; D.ext_hi = v[1] > v[0] ? v[1] : v[0]; D.ext_valid = 1;
    }
    *lo = D.ext_lo; *hi = D.ext_hi;
    return BCFGPU_OK;
}

extern "C" int bcfgpu_pool_upload(bcfgpu_ctx *ctx, const bcfgpu_reads *rd, const bcfgpu_packed *pk, const uint8_t *r_mapq)
{
    const int rc = pool_upload_impl("bcfgpu_pool_upload", ctx, rd, pk, r_mapq);
    if (rc) return rc;
    // the arrays are the caller's: they are free again when this call returns (bcfgpu_pileup[_packed] wait later, with the counts)
    hipStream_t stream = nullptr;
    bcfgpu_internal_device(ctx, &stream, nullptr);
    if (hipStreamSynchronize(stream) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_pool_upload: upload");
    return BCFGPU_OK;
}

// The read callback running ahead of the column loop (mpileup.c:183-246): the next region's pool comes up on the copy stream while
// the stages of the current one run on the context's.  Nothing of the current pool is touched: the copies go to the other set.
extern "C" int bcfgpu_pool_stage(bcfgpu_ctx *ctx, const bcfgpu_reads *rd, const bcfgpu_packed *pk, const uint8_t *r_mapq)
{
    const char *who = "bcfgpu_pool_stage";
    if (const int rc = pool_check_args(who, ctx, rd, pk, r_mapq)) return rc;
    if (bcfgpu_internal_device(ctx, nullptr, nullptr)) return pool_fail(who, BCFGPU_E_ARG, "bad context");
    PoolStage *st = bcfgpu_internal_pool_stage(ctx, true);
    if (!st) return pool_fail(who, BCFGPU_E_HIP, "copy stream");
    // a staged pool nobody adopted is replaced: its copies write to the buffers this call reuses (and may regrow)
    if (st->pending) {
        st->pending = 0;
        if (hipEventSynchronize(st->copied) != hipSuccess) return pool_fail(who, BCFGPU_E_HIP, "the staged copies");
    }
    // the other set held the pool before the last adopt, and that adopt's kernels read the staging slots: behind both
    if (st->freed_valid && hipStreamWaitEvent(st->copy, st->freed, 0) != hipSuccess) return pool_fail(who, BCFGPU_E_HIP, "hipStreamWaitEvent");
    const int rc = pool_copy(who, ctx, rd, pk, r_mapq, POOL_SET[st->set ^ 1], PACKED_STAGED, st->copy, *st);
    if (rc) { hipStreamSynchronize(st->copy); return rc; }          // (the caller's arrays are its own again after a failure)
    if (hipEventRecord(st->copied, st->copy) != hipSuccess) { hipStreamSynchronize(st->copy); return pool_fail(who, BCFGPU_E_HIP, "hipEventRecord"); }
    st->pending = 1;
    return BCFGPU_OK;
}

extern "C" int bcfgpu_pool_adopt(bcfgpu_ctx *ctx)
{
    const char *who = "bcfgpu_pool_adopt";
    hipStream_t stream = nullptr;
    if (!ctx || bcfgpu_internal_device(ctx, &stream, nullptr)) return pool_fail(who, BCFGPU_E_ARG, "bad context");
    PoolStage *st = bcfgpu_internal_pool_stage(ctx, false);
    if (!st->pending) return pool_fail(who, BCFGPU_E_ARG, "no staged read pool on this context (bcfgpu_pool_stage)");
    // the caller's arrays are free again when this call returns: the copies' event, not the context's stream
    if (hipEventSynchronize(st->copied) != hipSuccess) return pool_fail(who, BCFGPU_E_HIP, "the staged copies");
    if (hipStreamWaitEvent(stream, st->copied, 0) != hipSuccess) return pool_fail(who, BCFGPU_E_HIP, "hipStreamWaitEvent");
    st->pending = 0;
    bcfgpu_internal_pool_replaced(ctx);
    st->set ^= 1;
    const int rc = pool_form(who, ctx, *st, stream);
    // what is queued on the context's stream up to here is all that reads the old pool's set and the staging slots
    st->freed_valid = hipEventRecord(st->freed, stream) == hipSuccess;
    if (!st->freed_valid) hipStreamSynchronize(stream);
    return rc;
}

extern "C" int bcfgpu_pool_keep(bcfgpu_ctx *ctx, const uint8_t *keep)
{
    hipStream_t stream = nullptr;
    if (!ctx || bcfgpu_internal_device(ctx, &stream, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_pool_keep: bad context");
    DevPool &D = *bcfgpu_internal_pool_state(ctx);
    if (!D.valid) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_pool_keep: no read pool on this context (bcfgpu_pool_upload)");
    if (!keep) { D.keep = nullptr; return BCFGPU_OK; }
    uint8_t *d = (uint8_t*)bcfgpu_internal_ws(ctx, WS_POOL_KEEP, (size_t)D.n_reads + 64);
    if (!d) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_pool_keep: device workspace");
    if (D.n_reads && hipMemcpyAsync(d, keep, (size_t)D.n_reads, hipMemcpyHostToDevice, stream) != hipSuccess)
        return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_pool_keep: upload");
    if (hipStreamSynchronize(stream) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_pool_keep: upload");   // (keep may be the caller's stack)
    D.keep = d;
    return BCFGPU_OK;
}

extern "C" int bcfgpu_pool_download(bcfgpu_ctx *ctx, uint8_t *qual, uint8_t *zq, uint8_t *r_mapq)
{
    hipStream_t stream = nullptr;
    if (!ctx || bcfgpu_internal_device(ctx, &stream, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_pool_download: bad context");
    const DevPool &D = *bcfgpu_internal_pool_state(ctx);
    if (!D.valid) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_pool_download: no read pool on this context (bcfgpu_pool_upload)");
    if (qual && D.n_bases && hipMemcpyAsync(qual, D.qual, D.n_bases, hipMemcpyDeviceToHost, stream) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_pool_download");
    if (zq && D.n_bases) {
        if (D.zq) { if (hipMemcpyAsync(zq, D.zq, D.n_bases, hipMemcpyDeviceToHost, stream) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_pool_download"); }
        else std::memset(zq, 0, D.n_bases);
    }
    if (r_mapq && D.n_reads && hipMemcpyAsync(r_mapq, D.r_mapq, (size_t)D.n_reads, hipMemcpyDeviceToHost, stream) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_pool_download");
    if (hipStreamSynchronize(stream) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_pool_download");
    return BCFGPU_OK;
}
