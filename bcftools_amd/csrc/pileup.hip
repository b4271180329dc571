// pileup.hip -- the pileup itself on the device: from the reads of a region (a flat pool, as bcfgpu_baq and
// bcfgpu_gap_prep take it) to the site x sample x read tile that bcfgpu_mpileup / bcfgpu_pipeline run on.
//
// In the reference this is htslib's bam_mplp iterator plus the per-read accessors of bcf_call_glfgen (mpileup.c:320-347,
// bam2bcf.c:170-236): every pileup column lists, per sample, the reads covering the position with their query offset,
// is_del / is_refskip and the following indel.  A host-built tile costs 5 bytes per (read, position) over PCIe; the read
// pool it is built from is ~30x smaller (a 100-bp read is in 100 columns), so building the tile in HBM takes the PCIe
// link out of the way of the kernels.
//
// Mapping: one lane per (site, sample) cell -- the same gather-by-cell shape as glfgen_kernel, no atomics.  The reads of
// a sample are in ascending position order (a sorted BAM), so the reads that can cover position x are the window
// [first read with pos > x - max_span, first read with pos > x): two binary searches, then a scan of ~depth
// candidates.  Pass 1 counts the covering reads of every cell, a prefix sum gives plp_off, pass 2 resolves every
// covering read's CIGAR at x (query offset, deletion / reference skip, indel after the position: htslib's
// resolve_cigar) and writes the packed records of bcfgpu_pack_read into the cell's slice, in read order.
//
// Defined here: ReadMeta and the pileup, entry and tile kernels; the entry points that build a pileup from the context's read pool
// (bcfgpu_pool_pileup, and bcfgpu_pileup[_packed], which bring the pool up first) and those that read the last one
// (bcfgpu_pileup_entries, bcfgpu_pileup_indel_tile, bcfgpu_gap_prep_tile).  The read pool itself is pool.hip's.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ctx.h"

namespace bcfgpu {

// what a pileup entry needs from its read, in one 32-byte record (two 16-byte gathers per entry instead of nine scalar
// ones); a read whose CIGAR is a single operation -- the common case -- needs no CIGAR access at all
struct ReadMeta {
    int32_t pos, end;               // reference span [pos, end)
    uint32_t seq_off, cig_off;
    uint16_t lq, ntot;              // query length; M/=/X/I bases (get_position's denominator)
    uint8_t ncig, bits, mapq, pad;  // bits: 1 reverse strand, 2 has a soft clip, 4 unmapped
    uint32_t cig0;                  // the first CIGAR operation
    uint32_t pad2;
};
static_assert(sizeof(ReadMeta) == 32, "one read = two 16-byte loads");

// first k in [lo, hi) with a[k] > x
__device__ __forceinline__ int upper_bound(const int32_t *a, int lo, int hi, int x)
{
    while (lo < hi) { const int m = (lo + hi) >> 1; if (a[m] > x) hi = m; else lo = m + 1; }
    return lo;
}

// htslib's resolve_cigar: what the pileup says about a read (reference start rpos, CIGAR cg[0 .. ncig)) at a reference position x
// inside its span: the query offset, whether x lies in a deletion / a reference skip, and the indel that follows x
__device__ __forceinline__ void resolve_cigar(const uint32_t *cg, int ncig, int rpos, int x, int &qpos, int &is_del, int &is_skip, int &indel)
{
    int rx = rpos, y = 0;
    qpos = 0; is_del = 0; is_skip = 0; indel = 0;
    for (int c = 0; c < ncig; ++c) {
        const int op = cg[c] & 0xf, l = (int)(cg[c] >> 4);
        if (op == 0 || op == 7 || op == 8) {
            if (x < rx + l) {
                qpos = y + (x - rx);
                if (x == rx + l - 1) {                       // last base of the block: what follows?
                    int cc = c + 1;
                    while (cc < ncig && (cg[cc] & 0xf) == 6) ++cc;   // pads
                    if (cc < ncig) {
                        const int nop = cg[cc] & 0xf;
                        if (nop == 1) {
                            indel = (int)(cg[cc] >> 4);
                            for (++cc; cc < ncig && ((cg[cc] & 0xf) == 1 || (cg[cc] & 0xf) == 6); ++cc)
                                if ((cg[cc] & 0xf) == 1) indel += (int)(cg[cc] >> 4);
                        } else if (nop == 2) indel = -(int)(cg[cc] >> 4);
                    }
                }
                break;
            }
            rx += l; y += l;
        } else if (op == 2 || op == 3) {
            if (x < rx + l) { qpos = y; is_del = 1; is_skip = op == 3; break; }
            rx += l;
        } else if (op == 1 || op == 4) y += l;
    }
}

// A workgroup owns PT_COLS consecutive columns x PT_SMPL consecutive samples.  Lanes that are neighbours in the column index
// walk the same reads of one sample one base apart: their record loads fall on the same cache lines and their base / quality
// bytes are consecutive (a lane per cell in cell order -- neighbours = different samples -- made every load of every lane a
// cache line of its own: 14 ms for the 16 384-column x 1000-sample region of bench.py --mode pileup, this mapping: see DESIGN 5).
// In the tile a column's PT_SMPL cells are one contiguous chunk (site-major plp_off): the records are collected in LDS chunk
// by chunk and written out as PT_COLS contiguous spans.
#ifndef PT_COLS
#define PT_COLS 16
#endif
#define PT_SMPL (256 / PT_COLS)
// entries a workgroup's 256 cells may hold for that (a lane's own stores would be 4 + 1 bytes per entry, 120 bytes apart
// from its neighbour's); beyond it the lanes store directly
#define PILEUP_LDS_CAP 9216

template <bool FILL>
__global__ __launch_bounds__(256) void pileup_kernel(const PileupParams P)
{
    __shared__ uint32_t s_rd[FILL ? PILEUP_LDS_CAP : 1];
    __shared__ uint8_t s_ep[FILL ? PILEUP_LDS_CAP : 4];
    __shared__ uint32_t s_cb[PT_COLS], s_lb[PT_COLS + 1];        // chunk begin in the tile; chunk begin in LDS (+ total)
    // Workgroups are dealt to the 8 XCDs round-robin, and each XCD has its own L2: every XCD gets a contiguous range of
    // (sample tile, column tile) pairs with the column tile running fastest, so that the workgroups in flight on one XCD
    // walk the same samples' reads a few columns apart and find them in that L2.
    const unsigned n_bt = (unsigned)((P.n_sites + PT_COLS - 1) / PT_COLS), n_work = n_bt * (unsigned)((P.n_smpl + PT_SMPL - 1) / PT_SMPL);
    const unsigned per_xcd = gridDim.x >> 3;             // (the grid is a multiple of 8)
    const unsigned w = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    const bool in_grid = w < n_work;
    const int st = in_grid ? (int)(w / n_bt) : 0, bt = in_grid ? (int)(w - (unsigned)st * n_bt) : 0;
    const int c_local = threadIdx.x & (PT_COLS - 1), s_local = threadIdx.x / PT_COLS;
    const int site = bt * PT_COLS + c_local, s = st * PT_SMPL + s_local;
    const bool live = in_grid && site < P.n_sites && s < P.n_smpl;
    const long cell = (long)site * P.n_smpl + s;
    bool staged = false;
    if (FILL) {
        if (threadIdx.x < PT_COLS) {
            const int st_site = bt * PT_COLS + (int)threadIdx.x;
            uint32_t b = 0, e = 0;
            if (in_grid && st_site < P.n_sites) {
                const long c0 = (long)st_site * P.n_smpl + st * PT_SMPL;
                const int s1 = min(st * PT_SMPL + PT_SMPL, P.n_smpl);
                b = P.cnt[c0]; e = P.cnt[(long)st_site * P.n_smpl + s1];
            }
            s_cb[threadIdx.x] = b;
            // exclusive prefix sum of the chunk sizes over the 16 lanes
            uint32_t v = e - b, inc = v;
            #pragma unroll
            for (int d = 1; d < PT_COLS; d <<= 1) { const uint32_t u = __shfl_up(inc, d, PT_COLS); if ((int)threadIdx.x >= d) inc += u; }
            s_lb[threadIdx.x] = inc - v;
            if (threadIdx.x == PT_COLS - 1) s_lb[PT_COLS] = inc;
        }
        __syncthreads();
        staged = s_lb[PT_COLS] <= PILEUP_LDS_CAP;
    }
    // (the PT_COLS lanes of a sample act together below: columns past the tile's edge walk along with the last column and
    // produce nothing)
    if (in_grid && s < P.n_smpl) {
    const int x = P.beg + min(site, P.n_sites - 1);
    const int lo0 = P.smpl_off[s], hi0 = P.smpl_off[s + 1];
    const int hi = upper_bound(P.s_pos, lo0, hi0, x);                    // reads starting at or before x
    const int lo = upper_bound(P.s_pos, lo0, hi, x - (FILL ? P.max_span : *P.d_span));   // ... that can still reach x
    if (!FILL) {
        uint32_t n = 0;
        for (int k = lo; k < hi; ++k) n += P.meta[k].end > x ? 1u : 0u;
        if (live) P.cnt[cell] = n;
        return;
    }
    // One walk for the sample's PT_COLS columns: from the first column's first candidate to the last column's last, every
    // lane testing the read against its own column.  The lanes then ask for the same record in the same trip (one cache line
    // for the group instead of one per lane whose own range starts a read or two later) and for neighbouring bytes.
    int lo_c = lo, hi_c = hi;
    #pragma unroll
    for (int d = 1; d < PT_COLS; d <<= 1) { lo_c = min(lo_c, __shfl_xor(lo_c, d)); hi_c = max(hi_c, __shfl_xor(hi_c, d)); }
    uint32_t o = live ? P.cnt[cell] : 0u;                                // plp_off after the scan
    if (staged) o = o - s_cb[c_local] + s_lb[c_local];

    // The walk over the sample's reads that can reach x, software-pipelined by hand: a read's record (two 16-byte loads) is
    // fetched one trip ahead, its base and quality bytes are requested in the trip that resolves its CIGAR and used two
    // trips later, so that a trip waits for loads issued one and two trips ago instead of three dependent ones in a row
    // (at three wavefronts per SIMD -- the LDS staging -- the wavefronts sat in s_waitcnt 70 % of their time).
    uint32_t any_indel = 0;                                              // entries of the cell that are followed by an indel
    const uint4 *meta4 = reinterpret_cast<const uint4*>(P.meta);
    uint4 n0 = make_uint4(0, 0, 0, 0), n1 = n0;                          // the record of read k, fetched ahead
    const int k_last = P.n_reads - 1;
    if (lo_c < hi_c) { n0 = meta4[2 * (size_t)lo_c]; n1 = meta4[2 * (size_t)lo_c + 1]; }
    // two entries in flight: what is known of the entry without the bytes (w, e), whether a base exists (h), the bytes.
    // (Two register sets for the records and two for the entries, the trips written out in pairs: a value that is moved
    // from one variable to the next at the end of a trip counts as used there, and the compiler waits for every load.)
    struct Pend { bool v, h; uint32_t w, e, nt, bq; };
    Pend qa = {false, false, 0, 0, 0, 0}, qb = qa;
    uint4 na0 = make_uint4(0, 0, 0, 0), na1 = na0;
    auto trip = [&](const int k, const uint4 &m0, const uint4 &m1, uint4 &f0, uint4 &f1, Pend &q) __attribute__((always_inline)) {
        // (fetched whether or not there is a next read, from a clamped index: a load under a condition makes the compiler
        // wait for all outstanding loads at the next use instead of counting them)
        const size_t kf = (size_t)min(k + 1, k_last);
        f0 = meta4[2 * kf]; f1 = meta4[2 * kf + 1];
        // Straight-line code for the common read (one aligned block), for every lane whether its read covers x or not (v0 says
        // so at the end); the walk over a longer CIGAR only when some lane of the wavefront needs it.  Nested per-lane
        // branches around both cases cost as many scalar instructions (exec masks) as the entry did vector ones.
        bool v0 = live && k < hi_c && (int)m0.x <= x && (int)m0.y > x, h0 = false;
        uint32_t w0 = 0, e0 = 0, idx = 0;
        {
            const int rpos = (int)m0.x, lq = (int)(m1.x & 0xffff), ntot = (int)(m1.x >> 16);
            const int ncig = (int)(m1.y & 0xff);
            const uint32_t bits = (m1.y >> 8) & 0xff, mapq = (m1.y >> 16) & 0xff, so = m0.z;
            int qpos = x - rpos, is_del = 0, is_skip = 0, indel = 0, edist = qpos + 1;
            const int op0 = m1.z & 0xf;
            const bool walk = v0 && !(ncig == 1 && (op0 == 0 || op0 == 7 || op0 == 8));
            if (__any(walk)) if (walk) {
                const uint32_t *cg = P.cig + m0.w;
                resolve_cigar(cg, ncig, rpos, x, qpos, is_del, is_skip, indel);
                any_indel += indel != 0 ? 1u : 0u;
                // get_position, bam2bcf.c:80-114
                int iread = 0;
                edist = qpos + 1;
                if (P.want_epos && (bits & 2))
                    for (int c = 0; c < ncig; ++c) {
                        const int op = cg[c] & 0xf, l = (int)(cg[c] >> 4);
                        if (op == 0 || op == 7 || op == 8 || op == 1) iread += l;
                        else if (op == 4) { iread += l; if (iread <= qpos) edist -= l; }
                    }
            }
            // the record of bcfgpu_pack_read, but for the base and its quality
            int tail = lq - 1 - qpos;
            if (tail > qpos) tail = qpos;
            tail = tail < 0 ? 0 : tail > 255 ? 255 : tail;
            w0 = mapq << 8 | ((bits & 1) ? BCFGPU_RD_REV : 0) | ((bits & 2) ? BCFGPU_RD_SCLIP : 0) | (is_del ? BCFGPU_RD_DEL : 0)
                    | ((is_skip || (bits & 4)) ? BCFGPU_RD_SKIP : 0) | (uint32_t)tail << 24;
            if (P.want_epos) {
                int e = (int)((double)edist / (ntot + 1) * BCFGPU_NPOS);
                e0 = (uint32_t)(e < 0 ? 0 : e > BCFGPU_NPOS - 1 ? BCFGPU_NPOS - 1 : e);
            }
            h0 = v0 && qpos >= 0 && qpos < lq;
            idx = h0 ? so + (uint32_t)qpos : 0u;
        }
        // the entry whose bytes were requested two trips ago
        if (q.v) {
            const uint32_t word = q.w | (q.h ? q.bq : 0u) | (q.h ? (q.nt & 15u) : 15u) << 16;
            if (staged) { s_rd[o] = word; s_ep[o] = (uint8_t)q.e; }
            else { P.rd[o] = word; P.epos[o] = (uint8_t)q.e; }
            ++o;
        }
        q.v = v0; q.h = h0; q.w = w0; q.e = e0;
        q.nt = P.seq16[idx]; q.bq = P.qual[idx];                          // (unconditional: the pool is never empty, see bcfgpu_pileup)
    };
    if (lo_c < hi_c)
    for (int k = lo_c; k < hi_c + 2; k += 2) {
        trip(k, n0, n1, na0, na1, qa);
        trip(k + 1, na0, na1, n0, n1, qb);
    }
    if (any_indel && live && P.col_indel) atomicAdd(&P.col_indel[site], any_indel);                // (the fill pass walks the CIGARs: once per entry)
    }
    if (FILL && staged) {
        __syncthreads();
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int c = wave; c < PT_COLS; c += 4) {
            const uint32_t gb = s_cb[c], lb = s_lb[c], n = s_lb[c + 1] - lb;
            for (uint32_t i = lane; i < n; i += 64) P.rd[gb + i] = s_rd[lb + i];
            // the bytes: single ones up to a 4-byte boundary of the output, then words, then the rest
            const uint32_t head = min((4u - (gb & 3u)) & 3u, n), nw = (n - head) >> 2, tail0 = head + 4 * nw;
            if ((uint32_t)lane < head) P.epos[gb + lane] = s_ep[lb + lane];
            for (uint32_t i = lane; i < nw; i += 64) {
                const uint8_t *b = s_ep + lb + head + 4 * i;
                *reinterpret_cast<uint32_t*>(P.epos + gb + head + 4 * i) = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
            }
            if ((uint32_t)lane < n - tail0) P.epos[gb + tail0 + lane] = s_ep[lb + tail0 + lane];
        }
    }
}

// The pileup entries of selected columns as bcf_call_gap_prep wants them (read, query offset, indel): the same walk as
// the fill pass over the cells of those columns only.  sel_off = exclusive prefix sum of the cells' counts.
struct EntriesParams {
    PileupParams P;
    int n_cols;
    const int32_t *cols;            // [n_cols] column indices
    uint32_t *sel_cnt;              // [n_cols*n_smpl + 1] counts, then offsets
    int32_t *e_read, *e_qpos, *e_indel;
};

// The entries of the cells of selected columns, a lane per cell: sel[ci*S + s] = off[cols[ci]*S + s + 1] - off[cols[ci]*S + s].
// `off` is an offset array of S cells a column, one element past the end: plp_off of the pileup, or the offsets this kernel and
// the scan made of an earlier selection (cols then index that selection's columns).
__global__ __launch_bounds__(256) void cell_counts_kernel(const uint32_t *off, const int32_t *cols, int n_cols, int S, uint32_t *sel)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n_cols * S) return;
    const int ci = (int)(i / S), s = (int)(i - (long)ci * S);
    const size_t cell = (size_t)cols[ci] * S + s;
    sel[i] = off[cell + 1] - off[cell];
}

// A wavefront per cell, a lane per candidate read; the covering reads keep their order through a ballot prefix count.
__global__ __launch_bounds__(256) void entries_kernel(const EntriesParams E)
{
    const PileupParams &P = E.P;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= (long)E.n_cols * P.n_smpl) return;
    const int ci = (int)(i / P.n_smpl), s = (int)(i - (long)ci * P.n_smpl), site = E.cols[ci];
    const int x = P.beg + site;
    const int lo0 = P.smpl_off[s], hi0 = P.smpl_off[s + 1];
    const int hi = upper_bound(P.s_pos, lo0, hi0, x);
    const int lo = upper_bound(P.s_pos, lo0, hi, x - P.max_span);
    uint32_t o = E.sel_cnt[i];
    for (int kb = lo; kb < hi; kb += 64) {
        const int k = kb + lane;
        bool covers = false;
        int qpos = 0, indel = 0, is_del, is_skip;
        if (k < hi) {
            const ReadMeta m = P.meta[k];
            covers = m.end > x;
            if (covers) resolve_cigar(P.cig + m.cig_off, m.ncig, m.pos, x, qpos, is_del, is_skip, indel);
        }
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(covers);
        if (covers) {
            const uint32_t at = o + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
            E.e_read[at] = P.s_read ? P.s_read[k] : k; E.e_qpos[at] = qpos; E.e_indel[at] = indel;
        }
        o += (uint32_t)__popcll(mask);
    }
}

// The records of selected columns copied into a tile of their own (the indel pass runs on the candidate columns only), a lane per cell
__global__ __launch_bounds__(256) void subtile_kernel(const EntriesParams E, uint32_t *rd_out, uint8_t *ep_out)
{
    const PileupParams &P = E.P;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)E.n_cols * P.n_smpl) return;
    const int ci = (int)(i / P.n_smpl), s = (int)(i - (long)ci * P.n_smpl);
    const long cell = (long)E.cols[ci] * P.n_smpl + s;
    const uint32_t b = P.cnt[cell], e = P.cnt[cell + 1];
    uint32_t o = E.sel_cnt[i];
    for (uint32_t k = b; k < e; ++k, ++o) { rd_out[o] = P.rd[k]; ep_out[o] = P.epos[k]; }
}

// bcf_call_gap_prep gives up on a column whose indel reads, pooled over the samples, are fewer than min_support or a smaller
// share of the column's reads than min_frac (bam2bcf_indel.c:150-154, the default: no -p / per_sample_flt) -- in a large
// cohort nearly every column has some read with an indel and nearly none passes.  gap_keep_kernel decides it from two numbers
// the pileup left per column, before any of the column's entries is listed.
// The candidate columns bcf_call_gap_prep goes on with: that pooled support filter and the compaction of the columns that
// pass it, in one workgroup (a tile has some ten thousand candidates; in a large cohort a hundredth of them passes).
// kcols[j] = the column, kidx[j] = its place in `cols`; n_keep[0] = how many.  use_filter = 0 (per_sample_flt): every column.
__global__ __launch_bounds__(1024) void gap_keep_kernel(const PileupParams P, const int32_t *cols, int n_cols, int use_filter, int min_support,
                                                        double min_frac, int32_t *kcols, int32_t *kidx, int32_t *n_keep)
{
    __shared__ int s_wave[16], s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n_cols; i0 += 1024) {
        const int i = i0 + tid;
        bool keep = false;
        long c = 0;
        if (i < n_cols) {
            c = cols[i];
            keep = true;
            if (use_filter) {
                const uint32_t n_alt = P.col_indel[c], n_tot = P.cnt[(c + 1) * P.n_smpl] - P.cnt[c * P.n_smpl];
                keep = !(n_tot == 0 || (double)n_alt / n_tot < min_frac || (int)n_alt < min_support);
            }
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
        if (lane == 0) s_wave[wave] = (int)__popcll(m);
        __syncthreads();
        int before = s_base;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        if (keep) { const int at = before + (int)__popcll(m & ((1ull << lane) - 1)); kcols[at] = (int32_t)c; kidx[at] = i; }
        __syncthreads();
        if (tid == 0) { int t = s_base; for (int w = 0; w < 16; ++w) t += s_wave[w]; s_base = t; }
        __syncthreads();
    }
    if (tid == 0) n_keep[0] = s_base;
}

// The indel pass's tile: the columns where bcf_call_gap_prep returned 0 (mpileup.c:354-360), picked from the columns the stage
// ran on.  lk[j] = the place of tile column j among those columns, lcols[j] = its column of the pileup; ksel = the entry offsets
// of the stage's columns, lsel = those of the tile's (cell_counts_kernel of ksel at lk, scanned).  The read records come from the
// pileup, the p->aux words from the stage's entry-ordered array.
__global__ __launch_bounds__(256) void live_tile_kernel(const PileupParams P, int n_live, const int32_t *lcols, const int32_t *lk, const uint32_t *ksel,
                                                        const uint32_t *lsel, const uint32_t *aux_in, uint32_t *rd_out, uint8_t *ep_out, uint32_t *aux_out)
{
    // a lane per (tile column, entry of the column): a column's entries are one stretch of the pileup, of the stage's array and of the tile
    for (int j = blockIdx.y; j < n_live; j += gridDim.y) {
        const size_t kc0 = (size_t)lk[j] * P.n_smpl;
        const uint32_t kb = ksel[kc0], n = ksel[kc0 + P.n_smpl] - kb;
        const uint32_t b = P.cnt[(size_t)lcols[j] * P.n_smpl], o = lsel[(size_t)j * P.n_smpl];
        for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n; k += gridDim.x * 256u) {
            rd_out[o + k] = P.rd[b + k]; ep_out[o + k] = P.epos[b + k]; aux_out[o + k] = aux_in[kb + k];
        }
    }
}

// One record per read (reference span, constants) from the caller's per-read arrays: a pass over the CIGARs, one lane per read
// of the (sample, position)-ordered list.  status[0] = the longest reference span, status[1] = 1: a read too long for the
// record's fields, 2: a sample's reads out of position order.
struct MetaParams {
    int n, n_smpl;
    const int32_t *r_pos, *r_lq, *r_flag, *r_ncig, *r_cig_off, *r_seq_off;
    const uint8_t *r_mapq;
    const uint8_t *keep;            // NULL, or [n] by pool index: 0 = the read does not enter the pileup
    const int32_t *s_read;          // pool index of sorted read k, or NULL: the pool is in that order already
    const int32_t *smpl_off;
    const uint32_t *cig;
    ReadMeta *meta; int32_t *s_pos; int *status;
};
__global__ __launch_bounds__(256) void pileup_meta_kernel(const MetaParams M)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    int span = 1, bad = 0;
    if (k < M.n) {
        const int r = M.s_read ? M.s_read[k] : k;
        const int pos = M.r_pos[r], ncig = M.r_ncig[r], lq = M.r_lq[r], flag = M.r_flag[r];
        const uint32_t coff = (uint32_t)M.r_cig_off[r];
        const uint32_t *cg = M.cig + coff;
        int x = pos, ntot = 0, scl = 0;
        for (int c = 0; c < ncig; ++c) {
            const int op = cg[c] & 0xf, l = (int)(cg[c] >> 4);
            if (op == 0 || op == 7 || op == 8) { x += l; ntot += l; }
            else if (op == 2 || op == 3) x += l;
            else if (op == 1) ntot += l;
            else if (op == 4) scl = 1;
        }
        if (lq > 65535 || lq < 0 || ntot > 65535 || ncig > 255 || ncig < 0) bad = 1;
        const bool out = M.keep && !M.keep[r];                      // dropped by the caller's filters: covers no column
        ReadMeta m;
        m.pos = pos; m.end = (bad || out) ? pos : x; m.seq_off = (uint32_t)M.r_seq_off[r]; m.cig_off = coff;
        m.lq = (uint16_t)lq; m.ntot = (uint16_t)ntot; m.ncig = (uint8_t)ncig;
        m.bits = (uint8_t)(((flag & 16) ? 1 : 0) | (scl ? 2 : 0) | ((flag & 4) ? 4 : 0));
        m.mapq = M.r_mapq[r]; m.pad = 0; m.cig0 = ncig > 0 ? cg[0] : 0; m.pad2 = 0;
        uint4 *o = reinterpret_cast<uint4*>(M.meta + k);
        const uint4 *mi = reinterpret_cast<const uint4*>(&m);
        o[0] = mi[0]; o[1] = mi[1];
        M.s_pos[k] = pos;
        if (!bad && !out) span = x - pos;
        if (k > 0) {
            const int rp = M.s_read ? M.s_read[k - 1] : k - 1;
            if (pos < M.r_pos[rp]) {                                     // fine only across a sample boundary
                const int idx = upper_bound(M.smpl_off, 0, M.n_smpl + 1, k);
                if (M.smpl_off[idx - 1] != k) bad |= 2;
            }
        }
    }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) { span = max(span, __shfl_xor(span, o)); bad |= __shfl_xor(bad, o); }
    if ((threadIdx.x & 63) == 0) {
        // (the maximum only grows: a wavefront that does not raise what is there already stays away from the word -- 77 000
        // wavefronts queueing on one address were most of this kernel's time)
        if (span > 1 && span > *reinterpret_cast<volatile int*>(&M.status[0])) atomicMax(&M.status[0], span);
        if (bad) atomicOr(&M.status[1], bad);
    }
}

// sum of the per-cell counts in 64 bits (grid-stride, one atomic per workgroup)
__global__ __launch_bounds__(256) void count_total_kernel(const uint32_t *cnt, size_t n, unsigned long long *tot)
{
    unsigned long long v = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) v += cnt[i];
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(tot, v);
}

// per column: its entries and how many of them are followed by an indel, two words a column
__global__ __launch_bounds__(256) void col_counts_kernel(const uint32_t *off, const uint32_t *col_indel, int n_sites, int S, uint32_t *out)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_sites) return;
    out[2 * k] = off[(size_t)(k + 1) * S] - off[(size_t)k * S];
    out[2 * k + 1] = col_indel[k];
}

// the per-read arrays bcfgpu_gap_prep takes (bcfgpu_reads), rebuilt from the pileup's read records; by pool index
__global__ __launch_bounds__(256) void gap_unpack_reads_kernel(const PileupParams P, int32_t *r_pos, int32_t *r_lq, int32_t *r_flag,
                                                               int32_t *r_ncig, int32_t *r_cig_off, int32_t *r_seq_off)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= P.n_reads) return;
    const ReadMeta m = P.meta[k];
    const int r = P.s_read ? P.s_read[k] : k;
    r_pos[r] = m.pos; r_lq[r] = m.lq; r_flag[r] = ((m.bits & 1) ? 16 : 0) | ((m.bits & 4) ? 4 : 0);
    r_ncig[r] = m.ncig; r_cig_off[r] = (int32_t)m.cig_off; r_seq_off[r] = (int32_t)m.seq_off;
}
__global__ __launch_bounds__(256) void gap_col_pos_kernel(const int32_t *cols, int n_cols, int beg, int32_t *pos)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_cols) pos[i] = beg + cols[i];
}

}  // namespace bcfgpu

using namespace bcfgpu;

static int no_workspace(const char *who) { return bcfgpu_set_error(BCFGPU_E_NOMEM, who, "device workspace"); }

// ---- bcfgpu_pool_pileup: the tile built from the context's read pool -------------------------------------------------
// bcfgpu_pileup / bcfgpu_pileup_packed = pool_upload_impl (pool.hip) + pool_pileup_impl.  The host part is argument checks, the
// read -> sample bookkeeping (one pass over r_smpl, none when the caller hands over smpl_off), the reference codes, and launches.

// seq_nt16_table restricted to what a reference sequence holds (IUPAC codes, case-insensitive; anything else is N)
static int ref_nt16(char c)
{
    static const char *codes = "=ACMGRSVTWYHKDBN";
    if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    for (int i = 1; i < 16; ++i) if (codes[i] == c) return i;
    return 15;
}

// (grow-only scratch kept per calling thread and page-locked: the upload of s_read is then a DMA transfer the call does not wait for)
struct PinnedScratch {
    void *p = nullptr; size_t bytes = 0; bool pinned = false;
    void drop() { if (p) { if (pinned) hipHostFree(p); else free(p); } p = nullptr; bytes = 0; }
    ~PinnedScratch() { if (p && !pinned) free(p); }              // (a pinned block outlives the runtime's teardown order: left to the process exit)
};

// Which reads belong to which sample (usually they come grouped: one file per sample).  smpl_off[0 .. S] = the samples' ranges in
// the (sample, position)-ordered list of the pool's n reads, from the caller's offsets or a pass over r_smpl; *s_read = the pool
// index of every read of that list, or NULL: the pool is in that order already.
static int sample_order(const char *who, int n, int S, const int32_t *r_smpl, const int32_t *given_off, hipStream_t stream,
                        std::vector<int32_t> &smpl_off, int32_t **s_read)
{
    auto fail = [&](int code, const char *what) { return bcfgpu_set_error(code, who, what); };
    smpl_off.assign(S + 1, 0);
    *s_read = nullptr;
    if (given_off) {
        for (int s = 0; s <= S; ++s) smpl_off[s] = given_off[s];
        if (smpl_off[0] != 0 || smpl_off[S] != n) return fail(BCFGPU_E_ARG, "smpl_off does not cover the pool");
        for (int s = 0; s < S; ++s) if (smpl_off[s + 1] < smpl_off[s]) return fail(BCFGPU_E_ARG, "smpl_off is not ascending");
        return BCFGPU_OK;
    }
    const int nthr = host_threads(n);
    std::vector<std::vector<int32_t>> t_cnt(nthr);
    std::vector<int> t_flag(nthr, 0);
    on_threads(nthr, [&](int t) {
        const int k0 = (int)((long)n * t / nthr), k1 = (int)((long)n * (t + 1) / nthr);
        std::vector<int32_t> &c = t_cnt[t];
        c.assign(S, 0);
        int flag = 0;
        for (int r = k0; r < k1; ++r) {
            const int sm = r_smpl[r];
            if (sm < 0 || sm >= S) { flag |= 1; continue; }
            if (r && sm < r_smpl[r - 1]) flag |= 2;
            ++c[sm];
        }
        t_flag[t] = flag;
    });
    bool grouped = true;
    for (int t = 0; t < nthr; ++t) {
        if (t_flag[t] & 1) return fail(BCFGPU_E_ARG, "sample index out of range");
        if (t_flag[t] & 2) grouped = false;
        for (int s = 0; s < S; ++s) smpl_off[s + 1] += t_cnt[t][s];
    }
    for (int s = 0; s < S; ++s) smpl_off[s + 1] += smpl_off[s];
    if (grouped) return BCFGPU_OK;
    // counting sort by sample, the given order kept inside a sample
    static thread_local PinnedScratch scratch;
    const size_t want = (size_t)n * 4 + 64;
    if (scratch.bytes < want) {
        hipStreamSynchronize(stream);                              // an earlier call's upload may still read the old block
        scratch.drop();
        const size_t sz = want + want / 8;
        if (hipHostMalloc(&scratch.p, sz, hipHostMallocDefault) == hipSuccess) scratch.pinned = true;
        else { (void)hipGetLastError(); scratch.p = malloc(sz); scratch.pinned = false; }
        scratch.bytes = scratch.p ? sz : 0;
        if (!scratch.p) return fail(BCFGPU_E_NOMEM, "host scratch");
    }
    *s_read = static_cast<int32_t*>(scratch.p);
    std::vector<int32_t> cur(smpl_off.begin(), smpl_off.end() - 1);
    for (int r = 0; r < n; ++r) (*s_read)[cur[r_smpl[r]]++] = r;
    return BCFGPU_OK;
}

// rd / epos (/ aux) of a tile of `total` entries in workspace `slot`, epos and aux at 256-byte-aligned offsets behind rd (aligned
// for 16-byte staging loads), and *t = the tile of n_sites columns with the offsets `off`.  ref16 == NULL: the zeros the caller left
// behind the offsets (the indel pass does not read it).
static int tile_layout(const char *who, bcfgpu_ctx *ctx, WsSlot slot, int n_sites, int S, const uint32_t *off, const int8_t *ref16,
                       size_t total, bool indel, bcfgpu_tile *t)
{
    const size_t ep_at = ((total + 4) * 4 + 255) & ~(size_t)255, aux_at = (ep_at + total + 64 + 255) & ~(size_t)255;
    uint8_t *d = (uint8_t*)bcfgpu_internal_ws(ctx, slot, indel ? aux_at + (total + 4) * 4 : ep_at + total + 64);
    if (!d) return no_workspace(who);
    t->n_sites = n_sites; t->is_indel = indel ? 1 : 0; t->n_reads = total;
    t->ref16 = ref16 ? ref16 : reinterpret_cast<const int8_t*>(off + (size_t)n_sites * S + 1);
    t->plp_off = off; t->rd = (const uint32_t*)d; t->epos = d + ep_at; t->aux = indel ? (const uint32_t*)(d + aux_at) : nullptr;
    return BCFGPU_OK;
}

// one bcfgpu_pool_pileup: what its device steps share
struct PlpBuild {
    const char *who; bcfgpu_ctx *ctx; hipStream_t stream;
    PileupParams P;
    size_t ncells; int grid;            // cells of the tile; workgroups of pileup_kernel
    bcfgpu_tile tile;                   // the tile, complete after plp_fill
};

// the inputs in HBM (the reference codes, the samples' ranges, the sorted order), the counters zeroed, one ReadMeta per read
static int plp_inputs(PlpBuild &B, const DevPool &D, const std::vector<int8_t> &ref16, const std::vector<int32_t> &smpl_off, const int32_t *s_read)
{
    bcfgpu_ctx *ctx = B.ctx; hipStream_t stream = B.stream;
    PileupParams &P = B.P;
    const int n = D.n_reads, n_sites = P.n_sites, S = P.n_smpl;
    B.tile.ref16 = (const int8_t*)ws_upload(ctx, WS_PLP_REF16, ref16.data(), (size_t)n_sites, 64, stream);
    P.smpl_off = (const int32_t*)ws_upload(ctx, WS_PLP_SMPL_OFF, smpl_off.data(), (size_t)(S + 1) * 4, 64, stream);
    MetaParams M{};
    M.n = n; M.n_smpl = S; M.smpl_off = P.smpl_off;
    M.r_pos = D.r_pos; M.r_lq = D.r_lq; M.r_flag = D.r_flag; M.r_ncig = D.r_ncig; M.r_cig_off = D.r_cig_off; M.r_seq_off = D.r_seq_off;
    M.r_mapq = D.r_mapq; M.keep = D.keep; M.cig = D.cig;
    M.s_read = s_read ? (const int32_t*)ws_upload(ctx, WS_PLP_S_READ, s_read, (size_t)n * 4, 64, stream) : nullptr;
    M.meta = (ReadMeta*)bcfgpu_internal_ws(ctx, WS_PLP_META, (size_t)n * sizeof(ReadMeta) + 64);
    M.s_pos = (int32_t*)bcfgpu_internal_ws(ctx, WS_PLP_S_POS, (size_t)n * 4 + 64);
    M.status = (int*)bcfgpu_internal_ws(ctx, WS_PLP_STATUS, 64);
    P.cig = D.cig; P.seq16 = D.seq16; P.qual = D.qual; P.s_read = M.s_read; P.meta = M.meta; P.s_pos = M.s_pos; P.d_span = M.status;
    uint32_t *d_cnt = (uint32_t*)bcfgpu_internal_ws(ctx, WS_PLP_CNT, (B.ncells + 1) * 4 + (size_t)n_sites * 4 + 64);
    if (!B.tile.ref16 || !P.smpl_off || (s_read && !M.s_read) || !M.meta || !M.s_pos || !M.status || !d_cnt) return no_workspace(B.who);
    P.cnt = d_cnt;
    P.col_indel = d_cnt + B.ncells + 1;
    BCFGPU_CHK(hipMemsetAsync(d_cnt, 0, (B.ncells + 1) * 4 + (size_t)n_sites * 4, stream));
    static const int init_status[2] = {1, 0};
    BCFGPU_CHK(hipMemcpyAsync(M.status, init_status, 8, hipMemcpyHostToDevice, stream));
    if (n) hipLaunchKernelGGL(pileup_meta_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, M);
    const int n_work = ((n_sites + PT_COLS - 1) / PT_COLS) * ((S + PT_SMPL - 1) / PT_SMPL);
    B.grid = (n_work + 7) / 8 * 8;                   // (a multiple of the XCD count: see the kernel's work mapping)
    return BCFGPU_OK;
}

// pass 1: the reads of every cell, their total, plp_off; the host waits here and learns the total, the longest span and what
// pileup_meta_kernel found wrong with the reads
static int plp_count(PlpBuild &B)
{
    auto fail = [&](int code, const char *what) { return bcfgpu_set_error(code, B.who, what); };
    hipStream_t stream = B.stream;
    PileupParams &P = B.P;
    uint32_t total = 0;
    int status[2] = {1, 0};
    if (B.ncells) {
        hipLaunchKernelGGL(pileup_kernel<false>, dim3(B.grid), dim3(256), 0, stream, P);
        // the total in 64 bits first: plp_off is 32-bit, a region whose pileup reaches 2^32 entries must be refused, not wrapped
        unsigned long long *d_tot64 = (unsigned long long*)bcfgpu_internal_ws(B.ctx, WS_PLP_TOTAL, 64);
        if (!d_tot64) return no_workspace(B.who);
        BCFGPU_CHK(hipMemsetAsync(d_tot64, 0, 8, stream));
        hipLaunchKernelGGL(count_total_kernel, dim3((unsigned)std::min<size_t>((B.ncells + 4095) / 4096, 1024)), dim3(256), 0, stream, P.cnt, B.ncells, d_tot64);   // (one atomic per wavefront on one word: few, long-running workgroups)
        // plp_off = exclusive prefix sum of the counts (in place, one element past the end for the total)
        if (const int rc = scan_exclusive(B.ctx, stream, WS_PLP_SCAN_TMP, P.cnt, (int)(B.ncells + 1))) return fail(rc, rc == BCFGPU_E_HIP ? "scan" : "device workspace");
        unsigned long long tot64 = 0;
        BCFGPU_CHK(hipMemcpyAsync(&total, P.cnt + B.ncells, 4, hipMemcpyDeviceToHost, stream));
        BCFGPU_CHK(hipMemcpyAsync(&tot64, d_tot64, 8, hipMemcpyDeviceToHost, stream));
        BCFGPU_CHK(hipMemcpyAsync(status, P.d_span, 8, hipMemcpyDeviceToHost, stream));
        BCFGPU_CHK(hipStreamSynchronize(stream));
        if (tot64 >> 32) return fail(BCFGPU_E_RANGE, "the region's pileup has 2^32 or more entries; use a smaller region per call");
    } else {
        BCFGPU_CHK(hipMemcpyAsync(status, P.d_span, 8, hipMemcpyDeviceToHost, stream));
        BCFGPU_CHK(hipStreamSynchronize(stream));
    }
    if (status[1] & 1) return fail(BCFGPU_E_RANGE, "a read is longer than 65535 bases or has more than 255 CIGAR operations");
    if (status[1] & 2) return fail(BCFGPU_E_ARG, "the reads of a sample are not in position order");
    P.max_span = status[0];
    B.tile.n_reads = total;
    return BCFGPU_OK;
}

// pass 2: the read records.  The scan's temporary storage is done with, its slot is reused (grow-only) for rd + epos.
static int plp_fill(PlpBuild &B)
{
    PileupParams &P = B.P;
    const size_t total = (size_t)B.tile.n_reads;
    if (const int rc = tile_layout(B.who, B.ctx, WS_PLP_RECS, P.n_sites, P.n_smpl, P.cnt, B.tile.ref16, total, false, &B.tile)) return rc;
    P.rd = const_cast<uint32_t*>(B.tile.rd); P.epos = const_cast<uint8_t*>(B.tile.epos);
    if (total) hipLaunchKernelGGL(pileup_kernel<true>, dim3(B.grid), dim3(256), 0, B.stream, P);
    BCFGPU_CHK(hipGetLastError());
    return BCFGPU_OK;
}

// Per column: its entries (the difference of two offsets, formed on the device: the offsets themselves are 4 bytes a cell and
// stay in HBM) and whether any is followed by an indel; two words a column come back, through page-locked memory.
static int plp_columns(PlpBuild &B, int32_t *col_n, uint8_t *col_indel)
{
    const PileupParams &P = B.P;
    const int n_sites = P.n_sites;
    if (!(col_n || col_indel) || !n_sites) return BCFGPU_OK;
    uint32_t *d_cc = (uint32_t*)bcfgpu_internal_ws(B.ctx, WS_PLP_COL_COUNTS, (size_t)n_sites * 8 + 64);
    uint32_t *h_cc = (uint32_t*)bcfgpu_internal_pinned(B.ctx, PIN_PLP_COL_COUNTS, (size_t)n_sites * 8 + 64);
    if (!d_cc || !h_cc) return no_workspace(B.who);
    hipLaunchKernelGGL(col_counts_kernel, dim3((n_sites + 255) / 256), dim3(256), 0, B.stream, P.cnt, P.col_indel, n_sites, P.n_smpl, d_cc);
    BCFGPU_CHK(hipMemcpyAsync(h_cc, d_cc, (size_t)n_sites * 8, hipMemcpyDeviceToHost, B.stream));
    BCFGPU_CHK(hipStreamSynchronize(B.stream));
    for (int k = 0; k < n_sites; ++k) {
        if (col_n) col_n[k] = (int32_t)h_cc[2 * k];
        if (col_indel) col_indel[k] = h_cc[2 * k + 1] ? 1 : 0;
    }
    return BCFGPU_OK;
}

static int pool_pileup_impl(const char *who, bcfgpu_ctx *ctx, const int32_t *r_smpl, const int32_t *given_off, int32_t beg, int32_t end,
                            const char *ref, int32_t ref_len, bcfgpu_tile *tile, int32_t *col_n, uint8_t *col_indel)
{
    auto fail = [&](int code, const char *what) { return bcfgpu_set_error(code, who, what); };
    if (!ctx || !tile || end < beg || (ref_len > 0 && !ref)) return fail(BCFGPU_E_ARG, "bad arguments");
    PlpBuild B{};
    B.who = who; B.ctx = ctx;
    if (bcfgpu_internal_device(ctx, &B.stream, nullptr)) return fail(BCFGPU_E_ARG, "bad context");
    const DevPool &D = *bcfgpu_internal_pool_state(ctx);
    if (!D.valid) return fail(BCFGPU_E_ARG, "no read pool on this context (bcfgpu_pool_upload)");
    if (D.n_reads && !r_smpl && !given_off) return fail(BCFGPU_E_ARG, "bad arguments");
    // the last pileup's tile and a draw plan made for it end here, whether or not this call succeeds
    bcfgpu_internal_pileup_built(ctx, PileupParams{});
    bcfgpu_internal_drop_plan(ctx, WS_PLP_RECS);
    const bcfgpu_cfg *cfg = bcfgpu_internal_cfg(ctx);
    const int n_sites = end - beg, S = cfg->n_smpl;
    B.ncells = (size_t)n_sites * S;
    std::memset(tile, 0, sizeof *tile);
    if (B.ncells >> 31) return fail(BCFGPU_E_RANGE, "region x samples too large for one tile");
    std::vector<int32_t> smpl_off;
    int32_t *s_read = nullptr;
    if (const int rc = sample_order(who, D.n_reads, S, r_smpl, given_off, B.stream, smpl_off, &s_read)) return rc;
    std::vector<int8_t> ref16(n_sites);
    for (int k = 0; k < n_sites; ++k) ref16[k] = (int8_t)(beg + k < ref_len ? ref_nt16(ref[beg + k]) : 15);
    PileupParams &P = B.P;
    P.n_sites = n_sites; P.n_smpl = S; P.beg = beg; P.max_span = 1; P.n_reads = D.n_reads; P.n_bases = D.n_bases;
    P.want_epos = (cfg->fmt_flag & (BCFGPU_INFO_RPB | BCFGPU_INFO_VDB)) ? 1 : 0;
    int rc = plp_inputs(B, D, ref16, smpl_off, s_read);
    if (!rc) rc = plp_count(B);
    if (!rc) rc = plp_fill(B);
    if (!rc) rc = plp_columns(B, col_n, col_indel);
    if (rc) return rc;
    P.ref_len = ref_len;
    bcfgpu_internal_pileup_built(ctx, P);            // for bcfgpu_pileup_entries, bcfgpu_pileup_indel_tile, bcfgpu_gap_prep_tile
    *tile = B.tile;
    return BCFGPU_OK;
}

extern "C" int bcfgpu_pileup(bcfgpu_ctx *ctx, const bcfgpu_reads *rd, const uint8_t *r_mapq, const int32_t *r_smpl,
                             int32_t beg, int32_t end, const char *ref, int32_t ref_len,
                             bcfgpu_tile *tile, int32_t *col_n, uint8_t *col_indel)
{
    if (!rd || !tile || (rd->n_reads > 0 && !r_smpl)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_pileup: bad arguments");
    const int rc = pool_upload_impl("bcfgpu_pileup", ctx, rd, nullptr, r_mapq);
    return rc ? rc : pool_pileup_impl("bcfgpu_pileup", ctx, r_smpl, nullptr, beg, end, ref, ref_len, tile, col_n, col_indel);
}

extern "C" int bcfgpu_pileup_packed(bcfgpu_ctx *ctx, const bcfgpu_reads *rd, const bcfgpu_packed *pk, const uint8_t *r_mapq,
                                    const int32_t *r_smpl, int32_t beg, int32_t end, const char *ref, int32_t ref_len,
                                    bcfgpu_tile *tile, int32_t *col_n, uint8_t *col_indel)
{
    if (!rd || !pk || !tile || (rd->n_reads > 0 && !r_smpl && !pk->smpl_off)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_pileup_packed: bad arguments");
    const int rc = pool_upload_impl("bcfgpu_pileup_packed", ctx, rd, pk, r_mapq);
    return rc ? rc : pool_pileup_impl("bcfgpu_pileup_packed", ctx, r_smpl, pk->smpl_off, beg, end, ref, ref_len, tile, col_n, col_indel);
}

extern "C" int bcfgpu_pool_pileup(bcfgpu_ctx *ctx, const int32_t *r_smpl, const int32_t *smpl_off, int32_t beg, int32_t end,
                                  const char *ref, int32_t ref_len, bcfgpu_tile *tile, int32_t *col_n, uint8_t *col_indel)
{
    return pool_pileup_impl("bcfgpu_pool_pileup", ctx, r_smpl, smpl_off, beg, end, ref, ref_len, tile, col_n, col_indel);
}

// ---- the readers of the last pileup: bcfgpu_pileup_entries, bcfgpu_pileup_indel_tile, bcfgpu_gap_prep_tile ----------------

// What the three start with: the context's stream and the parameters of the last bcfgpu_pool_pileup, refused when there is none,
// when the read pool it was built from is gone, or when a column is not one of its columns.  `tile` != NULL: the tile the caller
// returned last (its records in workspace `recs`) ends here, and *tile starts as zeros.
static int last_pileup(const char *who, bcfgpu_ctx *ctx, int n_cols, const int32_t *cols, WsSlot recs, bcfgpu_tile *tile,
                       hipStream_t *stream, PileupParams *P)
{
    if (bcfgpu_internal_device(ctx, stream, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, who, "bad context");
    *P = *bcfgpu_internal_pileup_state(ctx);
    if (!P->cnt) return bcfgpu_set_error(BCFGPU_E_ARG, who, "no bcfgpu_pileup on this context yet");
    if (bcfgpu_internal_pileup_pool_gone(ctx))
        return bcfgpu_set_error(BCFGPU_E_ARG, who, "the read pool the last bcfgpu_pileup was built from is gone (replaced by bcfgpu_pool_upload / bcfgpu_pileup)");
    if (tile) {
        bcfgpu_internal_drop_plan(ctx, recs);
        std::memset(tile, 0, sizeof *tile);
    }
    for (int i = 0; i < n_cols; ++i)
        if (cols[i] < 0 || cols[i] >= P->n_sites) return bcfgpu_set_error(BCFGPU_E_ARG, who, "column out of range");
    return BCFGPU_OK;
}

// The cells of columns cols[0 .. n_cols) (in HBM) of the offsets `off`, S cells a column: *sel = workspace `sel_slot` with their
// counts, scanned in place over one more element -- sel[n_cols*S] is the total, its copy to *total is queued (total == NULL: none) --
// and zeros behind it for a tile's ref16.  Everything is queued on `stream`; the caller waits.  The scan takes workspace `tmp_slot`.
static int count_cells(const char *who, bcfgpu_ctx *ctx, hipStream_t stream, const uint32_t *off, const int32_t *cols, int n_cols, int S,
                       WsSlot sel_slot, WsSlot tmp_slot, uint32_t **sel, uint32_t *total)
{
    const size_t nsel = (size_t)n_cols * S, bytes = (nsel + 1) * 4 + (size_t)n_cols + 64;
    uint32_t *d_sel = *sel = (uint32_t*)bcfgpu_internal_ws(ctx, sel_slot, bytes);
    if (!d_sel) return no_workspace(who);
    BCFGPU_CHK(hipMemsetAsync(d_sel, 0, bytes, stream));
    if (!nsel) return BCFGPU_OK;
    hipLaunchKernelGGL(cell_counts_kernel, dim3((unsigned)((nsel + 255) / 256)), dim3(256), 0, stream, off, cols, n_cols, S, d_sel);
    if (const int rc = scan_exclusive(ctx, stream, tmp_slot, d_sel, (int)(nsel + 1))) return bcfgpu_set_error(rc, who, rc == BCFGPU_E_HIP ? "scan" : "device workspace");
    if (total) BCFGPU_CHK(hipMemcpyAsync(total, d_sel + nsel, 4, hipMemcpyDeviceToHost, stream));
    return BCFGPU_OK;
}

extern "C" int bcfgpu_pileup_entries(bcfgpu_ctx *ctx, int32_t n_cols, const int32_t *cols, int32_t *smpl_off,
                                     int32_t *p_read, int32_t *p_qpos, int32_t *p_indel, int64_t cap)
{
    const char *who = "bcfgpu_pileup_entries";
    if (!ctx || n_cols < 0 || (n_cols && (!cols || !smpl_off))) return bcfgpu_set_error(BCFGPU_E_ARG, who, "bad arguments");
    hipStream_t stream = nullptr;
    EntriesParams E{};
    if (const int rc = last_pileup(who, ctx, n_cols, cols, WS_ENT_OUT, nullptr, &stream, &E.P)) return rc;
    if (n_cols == 0) return BCFGPU_OK;
    const size_t nsel = (size_t)n_cols * E.P.n_smpl;
    int32_t *d_cols = (int32_t*)bcfgpu_internal_ws(ctx, WS_ENT_COLS, (size_t)n_cols * 4 + 16);
    if (!d_cols) return no_workspace(who);
    BCFGPU_CHK(hipMemcpyAsync(d_cols, cols, (size_t)n_cols * 4, hipMemcpyHostToDevice, stream));
    E.n_cols = n_cols; E.cols = d_cols;
    if (const int rc = count_cells(who, ctx, stream, E.P.cnt, d_cols, n_cols, E.P.n_smpl, WS_ENT_SEL, WS_ENT_SCAN_TMP, &E.sel_cnt, nullptr)) return rc;
    std::vector<uint32_t> off(nsel + 1);
    BCFGPU_CHK(hipMemcpyAsync(off.data(), E.sel_cnt, (nsel + 1) * 4, hipMemcpyDeviceToHost, stream));
    BCFGPU_CHK(hipStreamSynchronize(stream));
    const uint32_t total = off[nsel];
    for (size_t i = 0; i <= nsel; ++i) smpl_off[i] = (int32_t)off[i];
    if ((int64_t)total > cap || (total && (!p_read || !p_qpos || !p_indel)))
        return bcfgpu_set_error(BCFGPU_E_RANGE, who, "the output arrays are too small (sum of col_n over the columns)");
    if (!total) return BCFGPU_OK;
    int32_t *d_e = (int32_t*)bcfgpu_internal_ws(ctx, WS_ENT_OUT, (size_t)total * 12 + 16);
    if (!d_e) return no_workspace(who);
    E.e_read = d_e; E.e_qpos = d_e + total; E.e_indel = d_e + 2 * (size_t)total;
    hipLaunchKernelGGL(entries_kernel, dim3((unsigned)((nsel + 3) / 4)), dim3(256), 0, stream, E);
    BCFGPU_CHK(hipGetLastError());
    BCFGPU_CHK(hipMemcpyAsync(p_read, E.e_read, (size_t)total * 4, hipMemcpyDeviceToHost, stream));
    BCFGPU_CHK(hipMemcpyAsync(p_qpos, E.e_qpos, (size_t)total * 4, hipMemcpyDeviceToHost, stream));
    BCFGPU_CHK(hipMemcpyAsync(p_indel, E.e_indel, (size_t)total * 4, hipMemcpyDeviceToHost, stream));
    BCFGPU_CHK(hipStreamSynchronize(stream));
    return BCFGPU_OK;
}

extern "C" int bcfgpu_pileup_indel_tile(bcfgpu_ctx *ctx, int32_t n_cols, const int32_t *cols, const uint32_t *aux, int64_t n_aux,
                                        bcfgpu_tile *tile)
{
    const char *who = "bcfgpu_pileup_indel_tile";
    if (!ctx || n_cols < 0 || (n_cols && !cols) || !tile || n_aux < 0 || (n_aux && !aux)) return bcfgpu_set_error(BCFGPU_E_ARG, who, "bad arguments");
    hipStream_t stream = nullptr;
    EntriesParams E{};
    if (const int rc = last_pileup(who, ctx, n_cols, cols, WS_ITILE_RECS, tile, &stream, &E.P)) return rc;
    const size_t nsel = (size_t)n_cols * E.P.n_smpl;
    int32_t *d_cols = (int32_t*)bcfgpu_internal_ws(ctx, WS_ITILE_COLS, (size_t)n_cols * 4 + 16);
    if (!d_cols) return no_workspace(who);
    BCFGPU_CHK(hipMemcpyAsync(d_cols, cols, (size_t)n_cols * 4, hipMemcpyHostToDevice, stream));
    E.n_cols = n_cols; E.cols = d_cols;
    uint32_t total = 0;
    if (const int rc = count_cells(who, ctx, stream, E.P.cnt, d_cols, n_cols, E.P.n_smpl, WS_ITILE_SEL, WS_ITILE_SCAN_TMP, &E.sel_cnt, &total)) return rc;
    if (nsel) BCFGPU_CHK(hipStreamSynchronize(stream));
    if ((int64_t)total != n_aux) return bcfgpu_set_error(BCFGPU_E_ARG, who, "aux must hold one word per entry of the columns");
    bcfgpu_tile t{};
    if (const int rc = tile_layout(who, ctx, WS_ITILE_RECS, n_cols, E.P.n_smpl, E.sel_cnt, nullptr, total, true, &t)) return rc;
    if (total) {
        hipLaunchKernelGGL(subtile_kernel, dim3((unsigned)((nsel + 255) / 256)), dim3(256), 0, stream, E, const_cast<uint32_t*>(t.rd), const_cast<uint8_t*>(t.epos));
        BCFGPU_CHK(hipGetLastError());
        BCFGPU_CHK(hipMemcpyAsync(const_cast<uint32_t*>(t.aux), aux, (size_t)total * 4, hipMemcpyHostToDevice, stream));
        BCFGPU_CHK(hipStreamSynchronize(stream));
    }
    *tile = t;
    return BCFGPU_OK;
}

// ---- bcf_call_gap_prep for candidate columns of the last bcfgpu_pileup, everything staying in HBM -------------------
// one bcfgpu_gap_prep_tile: the call's arguments and what its steps hand on
struct GapTile {
    const char *who; bcfgpu_ctx *ctx; hipStream_t stream;
    PileupParams P;
    int n_cols; const int32_t *cols; const bcfgpu_reads *reads; const bcfgpu_indel_in *par; const bcfgpu_indel_out *out; int inscns_cap;
    int32_t *d_kcols, *h_k;             // the columns that go on, in HBM; [0] their number, [16 ..] their places in cols (pinned)
    int nk; std::vector<int32_t> kidx;  // ... on the host, after the first wait
    DevPool V;                          // the pileup's reads as bcfgpu_gap_prep's kernels index them, a view
    EntriesParams E; uint32_t total;    // the kept columns' entries
    int32_t *d_pos; char *d_ref; long ref_lo, ref_hi;
    uint32_t *d_aux;                    // p->aux by entry, as the stage leaves it
    std::vector<int32_t> lk, lcols;     // the columns where the stage returned 0: their places among the kept columns, their columns
};
#define GWS(slot, bytes) bcfgpu_internal_ws(T.ctx, slot, (bytes) + 64)      /* (padded as bcfgpu_gap_prep pads them) */
static float ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// every column starts as "bcf_call_gap_prep returned -1": the columns the stage goes on with overwrite their rows (gt_stage)
static void gt_outputs_start(const GapTile &T)
{
    const bcfgpu_indel_out *out = T.out;
    const int n_cols = T.n_cols;
    for (int i = 0; i < n_cols; ++i) { out->ret[i] = -1; for (int t = 0; t < 4; ++t) out->indel_types[(size_t)i * 4 + t] = 10000; }
    if (out->inscns) std::memset(out->inscns, 0, (size_t)n_cols * 4 * T.inscns_cap);
    if (out->maxins) std::memset(out->maxins, 0, (size_t)n_cols * 4);
    if (out->indelreg) std::memset(out->indelreg, 0, (size_t)n_cols * 4);
    if (out->max_support) std::memset(out->max_support, 0, (size_t)n_cols * 4);
    if (out->max_frac) std::memset(out->max_frac, 0, (size_t)n_cols * 4);
}

// The columns the stage goes on with: those that pass the pooled support filter (bam2bcf_indel.c:150-154; every column with
// per_sample_flt), compacted on the device.  Nothing after it touches a column that fails: no entry of it is listed, no workgroup
// of the stage is started for it.
static int gt_keep_columns(GapTile &T)
{
    const int n_cols = T.n_cols;
    int32_t *d_cols = (int32_t*)bcfgpu_internal_ws(T.ctx, WS_GTILE_COLS, (size_t)n_cols * 12 + 64);     // cols, then the kept columns, then their places in cols
    int32_t *d_nk = (int32_t*)bcfgpu_internal_ws(T.ctx, WS_GTILE_N_KEPT, 64);
    T.h_k = (int32_t*)bcfgpu_internal_pinned(T.ctx, PIN_GTILE_KEPT, (size_t)n_cols * 4 + 64);
    if (!d_cols || !d_nk || !T.h_k) return no_workspace(T.who);
    int32_t *d_kidx = d_cols + 2 * (size_t)n_cols;
    T.d_kcols = d_cols + n_cols;
    BCFGPU_CHK(hipMemcpyAsync(d_cols, T.cols, (size_t)n_cols * 4, hipMemcpyHostToDevice, T.stream));
    hipLaunchKernelGGL(gap_keep_kernel, dim3(1), dim3(1024), 0, T.stream, T.P, d_cols, n_cols, (!T.par->per_sample_flt && T.P.col_indel) ? 1 : 0,
                       T.par->min_support, T.par->min_frac, T.d_kcols, d_kidx, d_nk);
    BCFGPU_CHK(hipMemcpyAsync(T.h_k, d_nk, 4, hipMemcpyDeviceToHost, T.stream));
    BCFGPU_CHK(hipMemcpyAsync(T.h_k + 16, d_kidx, (size_t)n_cols * 4, hipMemcpyDeviceToHost, T.stream));
    return BCFGPU_OK;
}

// the reads as bcfgpu_gap_prep's kernels index them: the per-read arrays rebuilt from ReadMeta, by pool index
static int gt_reads_view(GapTile &T)
{
    const PileupParams &P = T.P;
    const int nr = P.n_reads;
    int32_t *d_rpos = (int32_t*)GWS(WS_VIEW_R_POS, (size_t)nr * 4), *d_rlq = (int32_t*)GWS(WS_VIEW_R_LQ, (size_t)nr * 4), *d_rflag = (int32_t*)GWS(WS_VIEW_R_FLAG, (size_t)nr * 4);
    int32_t *d_rncig = (int32_t*)GWS(WS_VIEW_R_NCIG, (size_t)nr * 4), *d_rcoff = (int32_t*)GWS(WS_VIEW_R_CIG_OFF, (size_t)nr * 4), *d_rsoff = (int32_t*)GWS(WS_VIEW_R_SEQ_OFF, (size_t)nr * 4);
    if (!d_rpos || !d_rlq || !d_rflag || !d_rncig || !d_rcoff || !d_rsoff) return no_workspace(T.who);
    if (nr) hipLaunchKernelGGL(gap_unpack_reads_kernel, dim3((nr + 255) / 256), dim3(256), 0, T.stream, P, d_rpos, d_rlq, d_rflag, d_rncig, d_rcoff, d_rsoff);
    DevPool &V = T.V;
    V.n_reads = nr;
    V.r_pos = d_rpos; V.r_lq = d_rlq; V.r_flag = d_rflag; V.r_ncig = d_rncig; V.r_cig_off = d_rcoff; V.r_seq_off = d_rsoff;
    V.cig = P.cig; V.seq16 = P.seq16; V.qual = const_cast<uint8_t*>(P.qual);
    return BCFGPU_OK;
}

// The kept columns' positions, the slice of the reference the batch touches, ZQ: queued behind the count of the columns' entries,
// whose total the host waits for next.
static int gt_site_inputs(GapTile &T)
{
    const PileupParams &P = T.P;
    const bcfgpu_reads *reads = T.reads;
    const int nk = T.nk, nr = P.n_reads;
    int cmin = INT32_MAX, cmax = 0;
    for (int j = 0; j < nk; ++j) { cmin = std::min(cmin, T.cols[T.kidx[j]]); cmax = std::max(cmax, T.cols[T.kidx[j]]); }
    T.d_pos = (int32_t*)GWS(WS_GAP_POS, (size_t)nk * 4);
    const int pmin = P.beg + cmin, pmax = P.beg + cmax;
    // The slice of the contig the batch touches.  The contig ends where bcfgpu_pileup was told it ends (ref_len): a candidate
    // column at or past that end reads nothing of par->ref (bcfgpu_indel_in carries no length of its own).
    const long ref_end = P.ref_len > 0 ? (long)P.ref_len : 0;
    const long ref_lo = std::min<long>(pmin > 65536 ? pmin - 65536 : 0, ref_end);
    const long ref_from = std::min<long>((long)pmax + 1, ref_end);
    const long ref_hi = ref_from + (long)strnlen(T.par->ref + ref_from, (size_t)std::min<long>(65536 + 4096, ref_end - ref_from));
    T.d_ref = (char*)GWS(WS_GAP_REF, (size_t)(ref_hi - ref_lo));
    T.ref_lo = ref_lo; T.ref_hi = ref_hi;
    const bool any_zq = reads && reads->zq && reads->r_has_zq;
    uint8_t *d_zq = any_zq ? (uint8_t*)GWS(WS_VIEW_ZQ, (size_t)P.n_bases) : nullptr, *d_haszq = any_zq ? (uint8_t*)GWS(WS_VIEW_HAS_ZQ, (size_t)nr) : nullptr;
    {   // no ZQ bytes from the host: those bcfgpu_pool_baq left in HBM, if the pool of the pileup is still the context's pool
        const DevPool &D = *bcfgpu_internal_pool_state(T.ctx);
        if (!any_zq && D.valid && D.zq && D.r_has_zq && D.n_reads == nr && D.seq16 == P.seq16) { d_zq = D.zq; d_haszq = D.r_has_zq; }
    }
    if (!T.d_pos || !T.d_ref || (any_zq && (!d_zq || !d_haszq))) return no_workspace(T.who);
    if (any_zq && reads->n_reads != nr) return bcfgpu_set_error(BCFGPU_E_ARG, T.who, "`reads` is not the pool of the last bcfgpu_pileup");
    hipLaunchKernelGGL(gap_col_pos_kernel, dim3((nk + 255) / 256), dim3(256), 0, T.stream, T.d_kcols, nk, P.beg, T.d_pos);
    if (ref_hi > ref_lo) BCFGPU_CHK(hipMemcpyAsync(T.d_ref, T.par->ref + ref_lo, (size_t)(ref_hi - ref_lo), hipMemcpyHostToDevice, T.stream));
    if (any_zq) {
        BCFGPU_CHK(hipMemcpyAsync(d_zq, reads->zq, (size_t)P.n_bases, hipMemcpyHostToDevice, T.stream));
        BCFGPU_CHK(hipMemcpyAsync(d_haszq, reads->r_has_zq, (size_t)nr, hipMemcpyHostToDevice, T.stream));
    }
    T.V.zq = d_zq; T.V.r_has_zq = d_haszq;
    return BCFGPU_OK;
}

// the kept columns' pileup entries (read, query offset, indel after the position), now that the host knows how many
static int gt_entries(GapTile &T)
{
    const size_t total = T.total;
    if ((T.total >> 31) != 0) return bcfgpu_set_error(BCFGPU_E_RANGE, T.who, "too many pileup entries in one call, use fewer columns");
    int32_t *d_e = (int32_t*)bcfgpu_internal_ws(T.ctx, WS_GTILE_ENT, total * 12 + 16);
    T.d_aux = (uint32_t*)GWS(WS_GAP_AUX, (total + 4) * 4);
    if (!d_e || !T.d_aux) return no_workspace(T.who);
    EntriesParams &E = T.E;
    E.e_read = d_e; E.e_qpos = d_e + total; E.e_indel = d_e + 2 * total;
    if (total) hipLaunchKernelGGL(entries_kernel, dim3((unsigned)(((size_t)T.nk * T.P.n_smpl + 3) / 4)), dim3(256), 0, T.stream, E);
    BCFGPU_CHK(hipGetLastError());
    return BCFGPU_OK;
}

// bcf_call_gap_prep on the kept columns (bcfgpu_internal_gap_core), its per-column results scattered to the caller's rows; the
// columns where it returned 0 are the indel pass's (lk, lcols)
static int gt_stage(GapTile &T, bcfgpu_gap_stats &gs, std::chrono::steady_clock::time_point t_begin)
{
    const bcfgpu_indel_out *out = T.out;
    const int nk = T.nk, inscns_cap = T.inscns_cap;
    GapIn g = gap_in_of(T.V, *T.par);
    g.n_sites = nk; g.n_smpl = T.P.n_smpl;
    g.pos = T.d_pos; g.smpl_off = reinterpret_cast<const int32_t*>(T.E.sel_cnt); g.p_read = T.E.e_read; g.p_qpos = T.E.e_qpos; g.p_indel = T.E.e_indel;
    g.ref = T.d_ref; g.ref_lo = T.ref_lo; g.ref_hi = T.ref_hi;
    gs.prepare_ms = ms_since(t_begin);
    // the stage's per-column results, by kept column
    std::vector<int32_t> k_ret(nk), k_types((size_t)nk * 4), k_maxins(nk), k_ireg(nk), k_msup(nk);
    std::vector<float> k_mfrac(nk);
    std::vector<int8_t> k_inscns(out->inscns ? (size_t)nk * 4 * inscns_cap : 0);
    bcfgpu_indel_out ko{};
    ko.ret = k_ret.data(); ko.indel_types = k_types.data(); ko.maxins = k_maxins.data(); ko.indelreg = k_ireg.data();
    ko.max_support = k_msup.data(); ko.max_frac = k_mfrac.data(); ko.inscns = out->inscns ? k_inscns.data() : nullptr;
    if (const int rc = bcfgpu_internal_gap_core(T.ctx, g, (size_t)T.total, T.d_aux, &ko, inscns_cap)) return rc;
    for (int j = 0; j < nk; ++j) {
        const size_t i = (size_t)T.kidx[j];
        out->ret[i] = k_ret[j];
        std::memcpy(out->indel_types + i * 4, &k_types[(size_t)j * 4], 16);
        if (out->inscns && inscns_cap) std::memcpy(out->inscns + i * 4 * inscns_cap, &k_inscns[(size_t)j * 4 * inscns_cap], (size_t)4 * inscns_cap);
        if (out->maxins) out->maxins[i] = k_maxins[j];
        if (out->indelreg) out->indelreg[i] = k_ireg[j];
        if (out->max_support) out->max_support[i] = k_msup[j];
        if (out->max_frac) out->max_frac[i] = k_mfrac[j];
        if (k_ret[j] == 0) { T.lk.push_back(j); T.lcols.push_back(T.cols[i]); }
    }
    return BCFGPU_OK;
}

// the indel pass's tile: the columns with ret == 0 (mpileup.c:354-360), their records from the pileup, p->aux from the stage
static int gt_live_tile(GapTile &T, bcfgpu_tile *tile)
{
    const int nl = (int)T.lk.size(), S = T.P.n_smpl;
    int32_t *d_l = (int32_t*)bcfgpu_internal_ws(T.ctx, WS_GTILE_LIVE, (size_t)nl * 8 + 64);
    if (!d_l) return no_workspace(T.who);
    BCFGPU_CHK(hipMemcpyAsync(d_l, T.lk.data(), (size_t)nl * 4, hipMemcpyHostToDevice, T.stream));
    BCFGPU_CHK(hipMemcpyAsync(d_l + nl, T.lcols.data(), (size_t)nl * 4, hipMemcpyHostToDevice, T.stream));
    uint32_t *d_lsel = nullptr, ltotal = 0;
    if (const int rc = count_cells(T.who, T.ctx, T.stream, T.E.sel_cnt, d_l, nl, S, WS_GTILE_LIVE_SEL, WS_GTILE_SCAN_TMP, &d_lsel, &ltotal)) return rc;
    BCFGPU_CHK(hipStreamSynchronize(T.stream));                 // (lk / lcols are this call's host vectors)
    bcfgpu_tile t{};
    if (const int rc = tile_layout(T.who, T.ctx, WS_GTILE_RECS, nl, S, d_lsel, nullptr, ltotal, true, &t)) return rc;
    if (ltotal) hipLaunchKernelGGL(live_tile_kernel, dim3(32, nl < 65535 ? nl : 65535), dim3(256), 0, T.stream, T.P, nl, d_l + nl, d_l, T.E.sel_cnt, d_lsel,
                                   (const uint32_t*)T.d_aux, const_cast<uint32_t*>(t.rd), const_cast<uint8_t*>(t.epos), const_cast<uint32_t*>(t.aux));
    BCFGPU_CHK(hipGetLastError());
    if (T.out->p_aux && ltotal) {                               // optional: the tile's p->aux words for the caller as well
        BCFGPU_CHK(hipMemcpyAsync(T.out->p_aux, t.aux, (size_t)ltotal * 4, hipMemcpyDeviceToHost, T.stream));
        BCFGPU_CHK(hipStreamSynchronize(T.stream));
    }
    *tile = t;
    return BCFGPU_OK;
}
#undef GWS

extern "C" int bcfgpu_gap_prep_tile(bcfgpu_ctx *ctx, int32_t n_cols, const int32_t *cols, const bcfgpu_reads *reads,
                                    const bcfgpu_indel_in *par, const bcfgpu_indel_out *out, int inscns_cap, bcfgpu_tile *tile)
{
    const char *who = "bcfgpu_gap_prep_tile";
    if (!ctx || n_cols < 0 || (n_cols && !cols) || !par || !par->ref || !out || !out->ret || !out->indel_types || !tile || inscns_cap < 0)
        return bcfgpu_set_error(BCFGPU_E_ARG, who, "bad arguments");
    GapTile T{};
    T.who = who; T.ctx = ctx; T.n_cols = n_cols; T.cols = cols; T.reads = reads; T.par = par; T.out = out; T.inscns_cap = inscns_cap;
    if (const int rc = last_pileup(who, ctx, n_cols, cols, WS_GTILE_RECS, tile, &T.stream, &T.P)) return rc;
    tile->is_indel = 1;
    bcfgpu_gap_stats &gs = *bcfgpu_internal_gap_stats(ctx);
    gs = bcfgpu_gap_stats{};
    if (n_cols == 0) return BCFGPU_OK;
    const auto t_begin = std::chrono::steady_clock::now();
    int rc;
    gt_outputs_start(T);
    if ((rc = gt_keep_columns(T)) || (rc = gt_reads_view(T))) return rc;                // (the reads are rebuilt while the columns are picked)
    BCFGPU_CHK(hipStreamSynchronize(T.stream));                 // the host waits: how many columns go on
    T.nk = T.h_k[0];
    T.kidx.assign(T.h_k + 16, T.h_k + 16 + T.nk);
    gs.prepare_ms = ms_since(t_begin);
    if (T.nk == 0) { gs.total_ms = ms_since(t_begin); return BCFGPU_OK; }
    T.E.P = T.P; T.E.n_cols = T.nk; T.E.cols = T.d_kcols;
    if ((rc = count_cells(who, ctx, T.stream, T.P.cnt, T.d_kcols, T.nk, T.P.n_smpl, WS_GTILE_SEL, WS_GTILE_SCAN_TMP, &T.E.sel_cnt, &T.total)) ||
        (rc = gt_site_inputs(T))) return rc;                    // (positions, reference and ZQ go up while the entries are counted)
    BCFGPU_CHK(hipStreamSynchronize(T.stream));                 // the host waits: the entry count sizes everything that follows
    if ((rc = gt_entries(T)) || (rc = gt_stage(T, gs, t_begin))) return rc;
    if (!T.lk.empty() && (rc = gt_live_tile(T, tile))) return rc;                       // (the host waits once more in there, for the tile's size)
    gs.total_ms = ms_since(t_begin);
    return BCFGPU_OK;
}

