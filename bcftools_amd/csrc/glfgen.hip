// glfgen.hip -- bcf_call_glfgen + errmod_cal for every (site,sample) cell of a tile.
//
// Replaces bam2bcf.c:147-258 and the errmod_cal() it calls (htslib errmod.c).
//
// A workgroup owns 256 consecutive (site,sample) cells, whose reads are one contiguous span of the `rd`/`epos`
// arrays (CSR order).  The work of bcf_call_glfgen's per-read loop splits by what it feeds:
//
//   phase A, one lane per READ (read-parallel, every lane busy whatever the depths of the cells):
//     the span is read straight from HBM, four consecutive reads per lane and trip (one 16-byte load of `rd`, one
//     4-byte load of `epos`), each input byte exactly once.  A wavefront's trip that lies whole inside its site segment
//     runs without byte masks, fetch guards and per-read key stores; the ragged ends run the general body.
//     Per read: the filters (bam2bcf.c:173-194), the quality
//     arithmetic (:196-203), and everything that only feeds SITE totals -- the I16 sums anno[4..15] (:221-226),
//     ori_depth, mq0 and the bias-test histograms (:228-252) -- which therefore never needs to know the read's cell:
//     per-lane partial sums, one reduction per workgroup and site.  What the cell needs of the read is 12 bits, left in
//     LDS as a u16 key at the read's position in the span:  strand | q<<1 | base<<7 | softclip<<10 | primary base<<11
//     (0 = read rejected).
//   phase B, one lane per CELL: the lane walks its own slice of keys: per-base counts, QS, ADF/ADR, DP4 counts and
//     errmod_cal, whose order-sensitive double sums are replayed in the reference's order (bit-identical results).
//
// LDS holds 2 bytes per read instead of the 5 of the raw tile, which is what lets four workgroups share a CU.
//
// errmod_cal() sorts the n 16-bit codes and walks them from the largest down.  Only the relative order of codes with
// the same base matters (per-base accumulators), and within a base the code order is the order of key7 = q<<1|strand:
// a counting pass per lane (count_runs) and a branch-free walk over the (quality, strand) runs (walk_runs).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "kernels.h"

namespace bcfgpu {

#define WG 256
#ifndef GLF_WAVES
#define GLF_WAVES 5          // wavefronts per SIMD the register budget is held to
#endif
#define DEF_MAPQ 20
#define CAP_DIST 25

// seq_nt16_int packed in nibbles: {4,0,1,4,2,4,4,4,3,4,4,4,4,4,4,4}
#define NT16_INT_TBL 0x4444444344424104ull
__device__ __forceinline__ int nt16_int(int c) { return (int)((NT16_INT_TBL >> (4 * (c & 15))) & 7); }
__host__ __device__ constexpr int tri(int j, int k) { return k * (k + 1) / 2 + j; }   // j<=k
// (j, k) of likelihood z = tri(j, k), z = 0..14, a nibble each (nibble 15: lanes past the last likelihood form (0, 0) and store nothing)
#define GLF_TRI_J 0x0432103210210100ull
#define GLF_TRI_K 0x0444443333222110ull
constexpr bool tri_tables_ok()
{
    int z = 0;
    for (int k = 0; k < 5; ++k) for (int j = 0; j <= k; ++j, ++z)
        if (tri(j, k) != z || (int)(GLF_TRI_J >> (4 * z) & 15) != j || (int)(GLF_TRI_K >> (4 * z) & 15) != k) return false;
    return z == 15 && (GLF_TRI_J >> 60) == 0 && (GLF_TRI_K >> 60) == 0;
}
static_assert(tri_tables_ok(), "GLF_TRI_J / GLF_TRI_K list (j, k) in the order of tri(j, k)");
// Lane l's value in every lane (every lane of the wavefront runs this).  ds_bpermute_b32, not v_readlane_b32: no vector ALU
// instruction, and the values stay out of the scalar registers, which the kernel is short of.
__device__ __forceinline__ uint32_t lane_u32(uint32_t x, int l) { return (uint32_t)__builtin_amdgcn_ds_bpermute(l << 2, (int)x); }
__device__ __forceinline__ double lane_f64(double x, int l)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return __longlong_as_double((long long)((unsigned long long)lane_u32((uint32_t)(u >> 32), l) << 32 | lane_u32((uint32_t)u, l)));
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// LDS layout (bytes): fk[264] f64 | slots[NSLOT][WG] u32 (a dword per quality rank) | hist [slots][HP_SIZE] 2 x u16 (the workgroup of a listed deep cell: [H_SIZE] i32) | site totals [slots][SITE_NSUM] u64 | keys u16[cap+8]
#define LDS_FK   0
#define LDS_CNT  2112
#ifndef NRANK
#define NRANK 10         // quality ranks a lane counts per round (count_runs): a dword each in LDS (9: 2.75, 10: 2.63, 11: 2.70 ms)
#endif
#define NSLOT    NRANK
#ifndef FU
#define FU       4         // source elements per trip of the slot counting
#endif
#define LDS_HIST_OFF (LDS_CNT + NSLOT * WG * 4)
// The workgroup's copy of a site's bias-test histograms, two 16-bit counters per dword: dword i < 220 = bin i of the REF arrays
// (kernels.h: POS, MQ, BQ) in the low half and of the ALT arrays in the high half; dword 220 + mq = the forward- and the
// reverse-strand mapQ histogram.  Half the LDS of plain counters, and the REF / ALT choice is the increment instead of an
// address.
// A half holds 65 535.  A workgroup's span can have more reads than that in one bin (256 cells of 257 reads with mapQ 60 will
// do: cells past 255 reads count every read), so the copy is added to the global histograms and cleared whenever the reads
// staged since it was last cleared, plus the window of the round that begins, could pass HP_MAX: a read adds at most one to
// a half, so no half passes HP_MAX (a window is at most GLF_MAX_WINDOW reads, kernels.h: csrc/api.hip sizes it).  The count
// is kept in LDS (s_pend) and looked at between two rounds, by every lane alike: a workgroup of one round, the rule, pays
// one store for it.  The mapQ >= 59 bins, which take whole rounds' counts at once, are not kept here: they go to the
// global histograms from the partial sums, as 32-bit counts.  The workgroup of a listed deep cell (one cell, one site,
// its reads in a single round of any length) keeps plain 32-bit counters in the same LDS, laid out as a site's global
// histograms.  (tests/test_gpu_site_stats.py: bins of exactly 65 535, 65 536 and up to 80 000 reads in every form.)
#define HP_SIZE 280
#define HP_MQS  220
#define HP_MAX  0xffffu
static_assert(GLF_MAX_WINDOW <= HP_MAX, "one round's window alone must fit a 16-bit half of the packed histograms");
static_assert(H_SIZE <= 2 * HP_SIZE, "a deep cell's 32-bit histograms take the LDS of two packed slots (hist_slots >= 2 whenever it is not 0)");
// per-lane partial sums of phase A: the I16 site totals anno[4..15], ori_depth and mq0 (site_sums[0..13]), then the reads of
// mapQ >= 59: all, REF base, reverse strand (the mapQ 59 bins of the four mapQ histograms).  csrc/api.hip sizes part_cols by it.
#define NPART 17
static_assert(NPART == SITE_NSUM + 3, "phase A's partial sums: the site totals and three mapQ >= 59 counts");

// the u16 key phase A leaves for phase B
#define KEY_PACK(rev, q, b, sc) ((uint32_t)(rev) | (uint32_t)(q) << 1 | (uint32_t)(b) << 7 | (uint32_t)(sc) << 10)
#define KEY_REV(k)  ((k) & 1u)
#define KEY_Q(k)    (((k) >> 1) & 63u)
#define KEY_B(k)    (((k) >> 7) & 7u)
#define KEY_SC(k)   (((k) >> 10) & 1u)
#define KEY_PRIM    0x800u     // the read shows the cell's primary base (the reference base; type 0 at indel sites)

// errmod_cal() sorts the cell's codes q<<5|strand<<4|base and walks them from the largest down; only the order among the
// reads of one base matters (per-base accumulators), and there the order is that of key7 = q<<1|reverse: quality by quality
// from the highest, the reverse-strand reads of a quality before its forward-strand ones.  The sort is replaced by counts:
// count_runs() leaves, in the lane's column of `s_slot`, one dword per distinct quality of the lane in descending order
// (rank r = qualities above it in the lane's mask):  reverse-strand reads | forward-strand reads << 8 | quality << 16.
// NRANK qualities per round (binned base qualities give a handful; a lane with more goes round again).
//   qm      bit q = some read of the source has quality q
//   src     the source: key(j) is its j-th key as phase A left it, ok(k) whether a key is one of its reads
// Returns sum of the qualities of the reads counted (QS).
#ifndef WR
#define WR 2            // reads of a run taken per step of the errmod walk
#endif
// the sources of count_runs(): the reads of the primary base (rejected reads are zeros), or those of the lane's other reads
// that show base b.  operator(): key7 of the j-th element, or -1 when it is not one of the source's reads.
struct PrimSrc {
    const uint16_t *kpp;
    __device__ __forceinline__ uint32_t key(int j) const { return kpp[j]; }
    __device__ __forceinline__ bool ok(uint32_t k) const { return k != 0; }
    __device__ __forceinline__ int operator()(int j) const { const uint32_t k = key(j); return ok(k) ? (int)(k & 0x7f) : -1; }
};
struct BaseSrc {
    const uint16_t *kp; int b;
    __device__ __forceinline__ uint32_t key(int i) const { return kp[i]; }
    __device__ __forceinline__ bool ok(uint32_t k) const { return KEY_B(k) == (uint32_t)b; }
    __device__ __forceinline__ int operator()(int i) const { const uint32_t k = key(i); return ok(k) ? (int)(k & 0x7f) : -1; }
};
__device__ __forceinline__ uint32_t popc64(uint64_t x) { return (uint32_t)__popc((uint32_t)x) + (uint32_t)__popc((uint32_t)(x >> 32)); }   // (32 bits wide: __popcll's compares are 64)
// The counting loop.  FIRST: the mask holds every quality of the source (the first round).  CHK: some lane of the wavefront has
// more than NRANK qualities in its mask, so a read's rank may lie beyond the slots.
template <bool FIRST, bool CHK, class Src>
__device__ __forceinline__ void count_keys(uint32_t *s_slot, uint64_t qm, int tid, Src src, int nsrc)
{
    const uint64_t qm1 = qm >> 1;                                   // rank of q = qualities above it = popcount(qm >> (q + 1))
    // FU source elements per trip, read whether or not they are inside the lane's slice (up to FU - 1 keys past it: other
    // cells' keys or the key array's slack): their reads are in flight before the first count is added, and whether an
    // element is the lane's own is one term of its count's condition.
    for (int j = 0; __any(j < nsrc); j += FU) {
        if (j < nsrc) {
            uint32_t k4[FU];
            #pragma unroll
            for (int u = 0; u < FU; ++u) k4[u] = src.key(j + u);
            #pragma unroll
            for (int u = 0; u < FU; ++u) {
                const uint32_t k = k4[u], q = KEY_Q(k);
                const uint32_t r = popc64(qm1 >> q);
                bool take = src.ok(k) && (u == 0 || j + u < nsrc);
                if (!FIRST) take = take && ((qm >> q) & 1ull);
                if (CHK) take = take && r < (uint32_t)NRANK;
                const uint32_t rv = (uint32_t)((int32_t)(k << 31) >> 31);                  // all ones on the reverse strand
                if (take) atomicAdd(&s_slot[r * WG + tid], (rv & 1u) | (~rv & 0x100u));     // reverse strand: 1, forward: 0x100
            }
        }
    }
}
template <bool FIRST, class Src>
__device__ __forceinline__ uint32_t count_runs(uint32_t *s_slot, uint64_t qm, int tid, Src src, int nsrc)
{
    #pragma unroll
    for (int k = 0; k < NRANK; ++k) s_slot[k * WG + tid] = 0;
    if (__any(popc64(qm) > (uint32_t)NRANK)) count_keys<FIRST, true>(s_slot, qm, tid, src, nsrc);
    else count_keys<FIRST, false>(s_slot, qm, tid, src, nsrc);
    // the quality of every rank joins its counts
    uint32_t qs = 0;
    uint64_t m = qm;
    #pragma unroll
    for (int r = 0; r < NRANK && __any(m != 0); ++r) {
        if (m != 0) {
            const uint32_t q = 63u - (uint32_t)__builtin_clzll(m);
            const uint32_t c = s_slot[r * WG + tid];                // reverse | forward << 8
            s_slot[r * WG + tid] = c | q << 16;
            qs = __builtin_amdgcn_udot4(c, q | q << 8, qs, false);  // + q * (reverse + forward)
            m &= ~(1ull << q);
        }
    }
    return qs;
}

// The descending walk of errmod_cal for one base over the runs count_runs() left: the t-th read of the lane adds
//     fk[reads of its strand so far] * beta[q][t][n]
// to the double sum, in the reference's order.  Every lane steps through its own runs, one read per step, in straight-line
// code (selects only: 64 lanes are at 64 different places of their runs); the loop runs for as many steps as the deepest
// cell of the wavefront has reads of the base, and a lane that is through adds fk = +0 times a finite table entry, which
// leaves its (non-negative) sum as it is.  The loads of a step are in flight while the step before is added; they are
// issued whether or not a lane still has a read (no branch around them: the compiler can then count the loads in flight
// and wait for the older one only).
// `brow`: byte offset of beta[0][0][n] (stored q, k, n: tables.cpp; the q = 0 row is all zeros).
template <class Src>
__device__ __forceinline__ double walk_runs(uint32_t *s_slot, uint64_t qm, const double *s_fk, const char *bbase, const double *pfx, int tid,
                                            uint32_t brow, Src src, int nsrc, uint32_t &rev_out, uint32_t &qs_out)
{
    double bs = 0;
    uint32_t qs = 0;
    uint32_t wpack = 0;      // reads walked so far: reverse strand in the low half, forward strand in the high half
    uint32_t cnt = 0;        // reads of the current quality still to walk, the same halves
    uint32_t koff = brow;    // brow + (reads walked so far) << 11: the k row of the next read
    uint32_t qoff = 0;       // current quality << 19
    uint32_t r = 0;          // ranks the lane has taken since the slots were filled
    uint32_t d_nx = 0;       // the dword of rank r, read ahead
    auto slot_of = [&](uint32_t rk) -> uint32_t { return s_slot[min(rk, (uint32_t)NRANK - 1u) * WG + tid]; };
    // One step = up to WR reads of the lane's current (quality, strand) run (binned base qualities make runs of several reads
    // the rule): the run bookkeeping is paid once for all of them.
    auto step = [&](uint32_t (&off)[WR], uint32_t (&wi)[WR]) -> bool {
        // the current quality is used up: the next rank (an empty dword past the lane's last one: the lane stays through)
        const bool pop = cnt == 0 && r < NRANK;
        cnt = pop ? (d_nx & 0xffu) | (d_nx & 0xff00u) << 8 : cnt;
        qoff = pop ? (d_nx & 0x3f0000u) << 3 : qoff;
        r += pop ? 1u : 0u;
        d_nx = slot_of(r);                                                // (the same dword again for a lane that did not pop)
        // reverse strand first
        const uint32_t sh = (cnt & 0xffffu) ? 0u : 16u;
        const uint32_t left = (cnt >> sh) & 0xffffu;                      // reads left in the run (0: the lane is through)
        const uint32_t w = (wpack >> sh) & 0xffffu;
        const uint32_t o1 = qoff + koff;
        #pragma unroll
        for (uint32_t u = 0; u < WR; ++u) {
            const bool act = left > u;
            wi[u] = act ? w + u : 256u;
            off[u] = act ? o1 + (u << 11) : brow;
        }
        const uint32_t took = min(left, (uint32_t)WR);
        wpack += took << sh; cnt -= took << sh;
        koff += took << 11;
        return __any(left != 0);
    };
    #define WALK_LOAD(B, F, off_, wi_) do { _Pragma("unroll") for (int u_ = 0; u_ < WR; ++u_) { \
        B[u_] = *reinterpret_cast<const double*>(bbase + (off_)[u_]); F[u_] = s_fk[(wi_)[u_]]; } } while (0)
    #define WALK_ADD(B, F) do { _Pragma("unroll") for (int u_ = 0; u_ < WR; ++u_) bs += F[u_] * B[u_]; } while (0)
    bool first = true;
    while (__any(qm != 0)) {                                              // a round: the next NRANK qualities of every lane
        qs += first ? count_runs<true>(s_slot, qm, tid, src, nsrc) : count_runs<false>(s_slot, qm, tid, src, nsrc);
        r = 0;
        d_nx = slot_of(0);
        // The first round starts from a sum of +0 with no read walked, so what the walk reaches after the lane's highest
        // quality depends on that quality, n and its two strand counts alone: pfx[q][n][reverse][forward] holds it, formed in
        // the walk's own order and arithmetic (glfgen_prefix_kernel), and the lane goes on from rank 1.  Selects only, no
        // branch: the load is issued for every lane and in every round (entry 0 for a lane outside the table, without a read
        // or in a later round), ahead of the first two steps' loads, and its value joins the sum behind them -- it is one more
        // load in flight, counted like the walk's own, and not waited for on its own.
        const uint32_t d0 = d_nx, r1 = d0 & 0xffu, f1 = (d0 >> 8) & 0xffu;
        const bool tb = first && brow < (uint32_t)GLF_PFX_N << 3 && (d0 & 0xe0e0u) == 0u && (d0 & 0xffffu) != 0u;
        const uint32_t ti = tb ? (d0 & 0x3f0000u) | brow << 7 | r1 << 5 | f1 : 0u;     // q << 16 | n << 10 | r << 5 | f
        const double t0 = pfx[ti];
        wpack = tb ? r1 | f1 << 16 : wpack;
        koff = tb ? brow + ((r1 + f1) << 11) : koff;
        r = tb ? 1u : 0u;
        d_nx = slot_of(r);
        first = false;
        // Two steps in flight, each in its own registers: a trip adds the older one and puts the step after next in its place, so
        // no step's operands are copied and the wait before an addition is for that step's loads alone.  (Once a step finds
        // no lane with a read, every later one adds +0: the two left over at the end are added in any order.)
        double bx[WR], fx[WR], by[WR], fy[WR];
        uint32_t off[WR], wi[WR];
        bool ax = step(off, wi);
        WALK_LOAD(bx, fx, off, wi);
        bool ay = step(off, wi);
        WALK_LOAD(by, fy, off, wi);
        bs = tb ? t0 : bs;
        while (ax) {
            WALK_ADD(bx, fx);
            ax = step(off, wi);
            WALK_LOAD(bx, fx, off, wi);
            if (!ay) break;
            WALK_ADD(by, fy);
            ay = step(off, wi);
            WALK_LOAD(by, fy, off, wi);
        }
        WALK_ADD(bx, fx);
        WALK_ADD(by, fy);
        // the qualities of this round leave the mask
        if (__any(__popcll(qm) > NRANK)) {
            uint64_t m = qm;
            for (int k = 0; k < NRANK && m; ++k) m &= ~(1ull << (63 - __clzll((long long)m)));
            qm = m;
        } else qm = 0;
    }
    #undef WALK_ADD
    #undef WALK_LOAD
    rev_out = wpack & 0xffffu; qs_out = qs;
    return bs;
}

// per-lane partial sums of phase A (one site segment of one staging round)
struct ReadSums {
    uint32_t t_bq, t_bq2, t_mq, t_mq2, t_md, t_md2;    // all accepted reads: baseQ, mapQ, min_dist and their squares
    uint32_t d_bq, d_bq2, d_mq, d_mq2, d_md, d_md2;    // the "diff" reads among them (is_diff of bam2bcf.c:186,195)
    __device__ __forceinline__ void clear() { t_bq = t_bq2 = t_mq = t_mq2 = t_md = t_md2 = d_bq = d_bq2 = d_mq = d_mq2 = d_md = d_md2 = 0; }
};
// per-lane counts of phase A (vector registers; added up with the partial sums once per site segment)
struct ReadCounts {
    uint32_t ori, mq0, m59, ref59, rev59;               // seen reads, mapQ 0, mapQ >= 59 (all / REF base / reverse strand)
    __device__ __forceinline__ void clear() { ori = mq0 = m59 = ref59 = rev59 = 0; }
};
typedef unsigned short v2u16 __attribute__((ext_vector_type(2)));

// Byte planes: the four reads of a lane side by side, read u in byte u of a dword.  Most of phase A works on the planes, a
// byte or a 16-bit half per read and four or two reads per instruction; flags are bit 7 of a read's byte ("80 masks").
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
#define SEL_EVEN 0x0c020c00u                   // plane -> reads 0 and 2 as the two u16 halves
#define SEL_ODD  0x0c030c01u                   // plane -> reads 1 and 3
#define SEL_JOIN 0x06020400u                   // perm(odd, even, SEL_JOIN): the two halves' low bytes back to a plane
#define SEL_GE8  0x07030501u                   // perm(odd, even, SEL_GE8): bit 8 of every half -> bit 0 of the read's byte
__device__ __forceinline__ v2u16 as_v2(uint32_t x) { return __builtin_bit_cast(v2u16, x); }
__device__ __forceinline__ uint32_t as_u(v2u16 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_min(as_v2(a), as_v2(b))); }
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_max(as_v2(a), as_v2(b))); }
// 0x80 in every byte that is not zero
__device__ __forceinline__ uint32_t nonzero80(uint32_t x) { return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }
// an 80 mask widened to whole bytes
__device__ __forceinline__ uint32_t bytes_of80(uint32_t m) { return m | (m - (m >> 7)); }
// byte u of x (u a constant)
__device__ __forceinline__ uint32_t byte_at(uint32_t x, int u) { return (x >> (8 * u)) & 0xffu; }
// A global load from a wave-uniform address plus a lane's byte offset: the address stays in scalar registers.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <typename T> struct GlobalWord { typedef T type; };
template <> struct GlobalWord<u32x4> { typedef uint4 type; };
template <typename T> __device__ __forceinline__ typename GlobalWord<T>::type load_global(const void *base, uint32_t off)
{
    typedef const __attribute__((address_space(1))) char *gbytes;
    typedef const __attribute__((address_space(1))) T *gptr;
    const T v = *(gptr)((gbytes)base + off);
    if constexpr (sizeof(T) == 16) return make_uint4(v.x, v.y, v.z, v.w); else return v;
}

// DEEP = false: the tile, 256 consecutive cells per workgroup.  A cell with more pileup entries than the LDS key window holds is
// not worked on here: it is listed (P.deep_*), and the launch that follows (DEEP = true) gives each listed cell a workgroup
// of its own -- phase A over the cell's reads with all 256 lanes, the keys in a global scratch array instead of LDS, phase B
// by the one lane that owns the cell.
template <bool INDEL, bool LDS_HIST, bool DEEP>
__global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(GLF_WAVES, GLF_WAVES))) void glfgen_kernel(const GlfgenParams P)
{
    extern __shared__ __align__(16) unsigned char smem[];
    if (DEEP && (blockIdx.x >= P.deep_ctr[0] || P.deep_list[2 * blockIdx.x] == 0xffffffffu)) return;
    const int cap = DEEP ? 0x7ffffff0 : P.lds_cap;
    double   *s_fk  = reinterpret_cast<double*>(smem + LDS_FK);
    uint32_t *s_cnt = reinterpret_cast<uint32_t*>(smem + LDS_CNT);
    int      *s_hist = reinterpret_cast<int*>(smem + LDS_HIST_OFF);
    unsigned long long *s_tot = reinterpret_cast<unsigned long long*>(s_hist + (size_t)P.hist_slots * HP_SIZE);   // [slots][SITE_NSUM]
    // phase A's per-lane partial sums [slots][NPART][pcol] share the slot counters' LDS: they are added up and cleared
    // before phase B takes the region
    uint32_t *s_part = s_cnt;
    const int pcol = P.part_cols;                    // columns per value: a power of two, NPART * slots * pcol <= 2048
    uint16_t *s_key = DEEP ? P.deep_keys + P.deep_list[2 * blockIdx.x + 1]
                           : reinterpret_cast<uint16_t*>(s_tot + (size_t)P.hist_slots * SITE_NSUM);
    __shared__ unsigned int s_next, s_skip, s_pend;
    constexpr bool PACKED = LDS_HIST && !DEEP;       // the histograms' LDS copy has two 16-bit counters per dword

    const int tid = threadIdx.x;
    const int S = P.n_smpl;
    const long ncells = (long)P.n_sites * S;
    const long cell0 = DEEP ? (long)P.deep_list[2 * blockIdx.x] : (long)blockIdx.x * WG;
    const long cell_end = DEEP ? cell0 + 1 : min(cell0 + WG, ncells);
    const int site0 = (int)(cell0 / S);
    const int site_last = (int)((cell_end - 1) / S);

    const long cell = cell0 + tid;
    const bool active = cell < cell_end;

    s_fk[tid] = P.fk[tid];
    if (tid < 8) s_fk[256 + tid] = 0.0;               // [256]: the factor of a lane that sits a chunk element out
    if (LDS_HIST) {
        for (int i = tid; i < P.hist_slots * HP_SIZE; i += WG) s_hist[i] = 0;
        for (int i = tid; i < P.hist_slots * SITE_NSUM; i += WG) s_tot[i] = 0;
    }

    int site = 0, ref4c = 4;
    uint32_t beg = 0, end = 0;
    if (active) {
        site = (int)(cell / S);
        beg = P.off[cell]; end = P.off[cell + 1];
        if (!INDEL) ref4c = nt16_int(P.ref16[site]);
    }
    const int primary = INDEL ? 0 : ref4c;            // the base most reads of the cell show
    uint32_t fmt_flag = (uint32_t)P.fmt_flag;
    asm volatile("" : "+s"(fmt_flag));
    const bool want_epos = (fmt_flag & (BCFGPU_INFO_RPB | BCFGPU_INFO_VDB)) != 0;
    const bool want_scr = (fmt_flag & (BCFGPU_INFO_SCR | BCFGPU_FMT_SCR)) != 0;
    const uint32_t span_end = P.off[cell_end];
    // The scalar arguments the inner loops use, as values of their own: read straight from the argument block they are
    // elements of one eight-register tuple, and when the scalar registers run short the whole tuple is spilled and brought
    // back, all eight, at every use inside phase A's loop.
    uint32_t n_reads_tot = P.n_reads, min_baseQ = (uint32_t)P.min_baseQ, capQ = (uint32_t)P.capQ;
    asm volatile("" : "+s"(n_reads_tot), "+s"(min_baseQ), "+s"(capQ));
    const uint32_t *p_rd = P.rd, *p_aux = P.aux, *p_off = P.off;          // (the same for the pointers of the inner loops)
    const uint8_t *p_epos = P.epos;
    asm volatile("" : "+s"(p_rd), "+s"(p_aux), "+s"(p_off), "+s"(p_epos));

    bool done = !active;
    // A cell must fit one staging round whatever its alignment (the window starts at a multiple of 4 reads).  One that does
    // not is listed for the launch that follows, with room for its keys in the scratch array; the rounds here step over its
    // reads.  Only when the list or the scratch array is full is the tile refused.
    bool deep = false;
    if (!DEEP && active && end - beg > (uint32_t)cap - 3u) {
        deep = true;
        const uint32_t need = (end - beg + 16u) & ~7u;           // keys of the cell, the slack of the 8-byte stores, a multiple of 8
        const uint32_t slot = atomicAdd(&P.deep_ctr[0], 1u), at = atomicAdd(&P.deep_ctr[1], need);
        const bool room = at + need <= P.deep_key_cap;
        if (slot < P.deep_cap) { P.deep_list[2 * slot] = room ? (uint32_t)cell : 0xffffffffu; P.deep_list[2 * slot + 1] = room ? at : 0u; }
        if (slot >= P.deep_cap || !room) { atomicExch(P.err, BCFGPU_E_DEPTH); atomicExch(&P.deep_ctr[2], 1u); }
    }
    uint32_t base = p_off[cell0];
    // s_pend: the reads staged since the packed histograms were last cleared, the window of the round that begins included
    if (PACKED && tid == 0) s_pend = min((base & ~3u) + (uint32_t)cap, span_end) - base;

    // the packed histograms of the workgroup's slots: added to the site's global ones and cleared
    auto flush_packed = [&](const bool clear) {
        const int nslot = min(P.hist_slots, P.n_sites - site0);
        for (int i = tid; i < nslot * HP_SIZE; i += WG) {
            const uint32_t v = (uint32_t)s_hist[i];
            if (!v) continue;
            if (clear) s_hist[i] = 0;
            const int sl = i / HP_SIZE, j = i - sl * HP_SIZE;
            int *g = P.hist + (long)(site0 + sl) * H_SIZE;
            const int lo = j < HP_MQS ? j : H_FWD_MQS + (j - HP_MQS), hi = j < HP_MQS ? j + H_ALT_OFF : H_REV_MQS + (j - HP_MQS);
            if (v & 0xffffu) atomicAdd(&g[lo], (int)(v & 0xffffu));
            if (v >> 16) atomicAdd(&g[hi], (int)(v >> 16));
        }
    };

    for (;;) {
        const uint32_t abase = base & ~3u;                       // key index 0 of this round
        const uint32_t lim = DEEP ? span_end : min(abase + (uint32_t)cap, span_end);
        if (tid == 0) { s_next = 0xffffffffu; s_skip = 0; }
        if (LDS_HIST) {
            int i0 = tid;                                        // the first dword's address is formed here, every round: hoisted out of
            asm volatile("" : "+v"(i0));                         // the rounds it is one more value alive through both phases, and spilled
            for (int i = i0; i < P.hist_slots * NPART * pcol; i += WG) s_part[i] = 0;
        }
        __syncthreads();
        const bool cand = !done && !deep && beg >= base && end <= lim;
        if (!done && !cand) atomicMin(&s_next, beg);             // the first cell left for a later round (deep tiles only): one that
        __syncthreads();                                         // does not fit the window any more, or a listed cell
        const uint32_t nb = s_next;
        const uint32_t rlim = min(nb, lim);                      // reads [base, rlim) belong to this round's cells
        const bool part = cand && end <= rlim;                   // this lane's cell is handled in this round (cells behind a listed cell wait)

        // ================= phase A: one lane per read =================
        for (int sg = site0; sg <= site_last; ++sg) {            // uniform: the site segments of the workgroup's span
            const long c_lo = max(cell0, (long)sg * S), c_hi = min(cell_end, (long)(sg + 1) * S);
            // (the same in every lane, but formed by the vector unit: handed to the scalar one, which chooses the trips below)
            const uint32_t rb = (uint32_t)__builtin_amdgcn_readfirstlane((int)max(p_off[c_lo], base));
            const uint32_t re = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(p_off[c_hi], rlim));
            if (rb >= re) continue;
            const int ref_base = INDEL ? -1 : (int)P.ref16[sg];
            const uint32_t ref4 = INDEL ? 4u : (uint32_t)nt16_int(ref_base);
            const uint32_t primq = INDEL ? 0u : ref4;            // `primary` of the segment's cells
            // nt16 code -> base 0..4 with code 0 ('=') standing for the reference base (bam2bcf.c:189-190)
            const unsigned long long tbl = (NT16_INT_TBL & ~0xfull) | (unsigned long long)ref4;
            int *hist = LDS_HIST ? s_hist + (sg - site0) * HP_SIZE : P.hist + (long)sg * H_SIZE;
            ReadSums A; A.clear();
            ReadCounts C; C.clear();
            // the constants of the planes: base 0..4 of a nt16 code by v_perm (codes 0..7 and 8..15, indexed by the low three
            // bits), the byte test baseQ >= min_baseQ (K + baseQ has bit 8 set), the segment's codes in every byte
            const uint32_t tlo_lo = 0x04010000u | ref4, tlo_hi = 0x04040402u, thi_lo = 0x04040403u, thi_hi = 0x04040404u;
            const uint32_t kq = 0x01000100u - min(min_baseQ, 256u) * 0x00010001u;
            const uint32_t cap2 = min(capQ, 0xffffu) * 0x00010001u;
            const uint32_t refb4 = (uint32_t)(ref_base & 15) * 0x01010101u, prim4 = primq * 0x01010101u;
            const uint32_t scm = want_scr ? 0x04040404u : 0u;
            const bool all_diff = !INDEL && ref4 >= 4;
            const bool no_ref = INDEL || ref_base < 0 || ref_base > 15;          // (isref below compares the nt16 codes)

            // Four consecutive reads of the lane, `vm4`: 0xff in the bytes of the reads inside [rb, re).  Per-lane control
            // flow only: any lane may run this on its own.
            auto quad = [&](const uint4 &w4, const uint4 &a4, uint32_t e4, uint32_t vm4, uint32_t &k01, uint32_t &k23) __attribute__((always_inline)) {
                // the rd words as byte planes: baseQ, mapQ, flags (nt16 | rev << 4 | sclip << 5 | DEL << 6 | SKIP << 7), min_dist
                const uint32_t t0 = perm(w4.y, w4.x, 0x05010400u), t1 = perm(w4.y, w4.x, 0x07030602u);
                const uint32_t t2 = perm(w4.w, w4.z, 0x05010400u), t3 = perm(w4.w, w4.z, 0x07030602u);
                uint32_t B4 = perm(t2, t0, 0x05040100u);
                const uint32_t M4 = perm(t2, t0, 0x07060302u);
                const uint32_t F4 = (vm4 & perm(t3, t1, 0x05040100u)) | (~vm4 & 0x80808080u);     // a read outside the segment: SKIP
                const uint32_t D4 = perm(t3, t1, 0x07060302u);
                uint32_t QR4, BB4;                                // q before the mapQ cap, base 0..4
                uint32_t ok80;
                const uint32_t seen80 = (INDEL ? F4 : F4 | F4 << 1) & 0x80808080u ^ 0x80808080u;   // !SKIP (SNP: and !DEL)
                if (INDEL) {
                    // the aux words: baseQ | seqQ << 8 | base << 16 (bam2bcf_indel.c:449-456), a read at a time
                    uint32_t qv[4], bv[4];
                    const uint32_t av[4] = { a4.x, a4.y, a4.z, a4.w }, wv[4] = { w4.x, w4.y, w4.z, w4.w };
                    #pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint32_t ax = av[u];
                        uint32_t b = (ax >> 16) & 0xf, q = ax & 0xff;
                        if (q < min_baseQ) { b = 0; q = wv[u] & 0xff; }
                        bv[u] = min(b, 4u);
                        qv[u] = min(q, (ax >> 8) & 0xff);
                    }
                    B4 = perm(perm(a4.w, a4.z, 0x04000c0cu), perm(a4.y, a4.x, 0x0c0c0400u), 0x07060100u);
                    QR4 = qv[0] | qv[1] << 8 | qv[2] << 16 | qv[3] << 24;
                    BB4 = bv[0] | bv[1] << 8 | bv[2] << 16 | bv[3] << 24;
                    ok80 = seen80;
                } else {
                    const uint32_t ge = perm(perm(0, B4, SEL_ODD) + kq, perm(0, B4, SEL_EVEN) + kq, SEL_GE8);
                    ok80 = seen80 & ge << 7;
                    QR4 = B4;
                    const uint32_t s = F4 & 0x07070707u;
                    BB4 = perm(perm(thi_hi, thi_lo, s), perm(tlo_hi, tlo_lo, s), 0x03020100u | (F4 >> 1 & 0x04040404u));
                }
                const uint32_t OK4 = bytes_of80(ok80);
                // mapQ: 255 -> DEF_MAPQ, then min(mapQ, capQ); two reads an instruction
                const uint32_t me = perm(0, M4, SEL_EVEN), mo = perm(0, M4, SEL_ODD);
                const uint32_t mfe = pk_min(me + (uint32_t)__mul24((int)perm(0, me + 0x00010001u, SEL_ODD), DEF_MAPQ - 255), cap2);
                const uint32_t mfo = pk_min(mo + (uint32_t)__mul24((int)perm(0, mo + 0x00010001u, SEL_ODD), DEF_MAPQ - 255), cap2);
                // q = clamp(min(q, mapQ), 4, 63)
                const uint32_t qe = pk_max(pk_min(pk_min(perm(0, QR4, SEL_EVEN), mfe), 0x003f003fu), 0x00040004u);
                const uint32_t qo = pk_max(pk_min(pk_min(perm(0, QR4, SEL_ODD), mfo), 0x003f003fu), 0x00040004u);
                const uint32_t Q4 = perm(qo, qe, SEL_JOIN);
                const uint32_t Mf4 = perm(mfo, mfe, SEL_JOIN);
                const uint32_t Df4 = perm(pk_min(perm(0, D4, SEL_ODD), 0x00190019u), pk_min(perm(0, D4, SEL_EVEN), 0x00190019u), SEL_JOIN);
                // the counts: seen reads, mapQ 0 and mapQ >= 59 of the accepted ones
                const uint32_t m59_80 = ok80 & perm(mfo + 0x00c500c5u, mfe + 0x00c500c5u, SEL_GE8) << 7;     // 59 + 197 = 256
                const uint32_t nref80 = no_ref ? 0x80808080u : nonzero80((F4 ^ refb4) & 0x0f0f0f0fu);      // nt != the reference's code
                C.ori += __builtin_popcount(seen80);
                C.mq0 += __builtin_popcount(ok80 & ~nonzero80(M4));
                C.m59 += __builtin_popcount(m59_80);
                C.ref59 += __builtin_popcount(m59_80 & ~nref80);
                C.rev59 += __builtin_popcount(m59_80 & F4 << 3);
                // the keys: byte lo = rev | q << 1 | base << 7, byte hi = base >> 1 | sclip << 2 | primary << 3; zero when rejected
                const uint32_t nprim80 = nonzero80(BB4 ^ prim4);
                const uint32_t klo = (((F4 >> 4) & 0x01010101u) | Q4 << 1 | (BB4 & 0x01010101u) << 7) & OK4;
                const uint32_t khi = (((BB4 >> 1) & 0x03030303u) | ((F4 >> 3) & scm) | ((nprim80 ^ 0x80808080u) >> 4)) & OK4;
                k01 = perm(khi, klo, 0x05010400u); k23 = perm(khi, klo, 0x07030602u);
                // the I16 sums: Σ x and Σ x² of the accepted reads, four reads a v_dot4_u32_u8
                const uint32_t Bm = B4 & OK4, Mm = Mf4 & OK4, Dm = Df4 & OK4;
                A.t_bq = __builtin_amdgcn_udot4(Bm, 0x01010101u, A.t_bq, false); A.t_bq2 = __builtin_amdgcn_udot4(Bm, Bm, A.t_bq2, false);
                A.t_mq = __builtin_amdgcn_udot4(Mm, 0x01010101u, A.t_mq, false); A.t_mq2 = __builtin_amdgcn_udot4(Mm, Mm, A.t_mq2, false);
                A.t_md = __builtin_amdgcn_udot4(Dm, 0x01010101u, A.t_md, false); A.t_md2 = __builtin_amdgcn_udot4(Dm, Dm, A.t_md2, false);
                const uint32_t dif80 = ok80 & (all_diff ? 0x80808080u : nprim80);                     // is_diff (bam2bcf.c:186,195)
                if (dif80) {                                      // rare: sequencing errors and the ALT reads of variant sites
                    const uint32_t DM = bytes_of80(dif80);
                    const uint32_t bd = Bm & DM, qd = Mm & DM, dd = Dm & DM;
                    A.d_bq = __builtin_amdgcn_udot4(bd, 0x01010101u, A.d_bq, false); A.d_bq2 = __builtin_amdgcn_udot4(bd, bd, A.d_bq2, false);
                    A.d_mq = __builtin_amdgcn_udot4(qd, 0x01010101u, A.d_mq, false); A.d_mq2 = __builtin_amdgcn_udot4(qd, qd, A.d_mq2, false);
                    A.d_md = __builtin_amdgcn_udot4(dd, 0x01010101u, A.d_md, false); A.d_md2 = __builtin_amdgcn_udot4(dd, dd, A.d_md2, false);
                }
                // bias-test histograms, a read at a time: ibq = (int)(baseQ/60.*60) is the identity on 0..59 (checked in tests).
                // The mapQ >= 59 bins of the four mapQ histograms (most reads) are the counts above; every ALT array sits
                // H_ALT_OFF after its REF array.
                #pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (!((ok80 >> (8 * u + 7)) & 1)) continue;
                    const bool isref = !((nref80 >> (8 * u + 7)) & 1), rev = (F4 >> (8 * u + 4)) & 1;
                    const uint32_t bq = byte_at(B4, u), mapQ = byte_at(Mf4, u), pos = byte_at(e4, u);
                    const bool m59 = (m59_80 >> (8 * u + 7)) & 1;
                    if (PACKED) {
                        const int inc = isref ? 1 : 0x10000;
                        atomicAdd(&hist[H_REF_POS + pos], inc);
                        atomicAdd(&hist[H_REF_BQ + min(bq, 59u)], inc);
                        if (!m59) {
                            atomicAdd(&hist[H_REF_MQ + mapQ], inc);
                            atomicAdd(&hist[HP_MQS + mapQ], rev ? 0x10000 : 1);
                        }
                    } else {
                        const uint32_t aoff = isref ? 0u : (uint32_t)H_ALT_OFF;
                        atomicAdd(&hist[aoff + H_REF_POS + pos], 1);
                        atomicAdd(&hist[aoff + H_REF_BQ + min(bq, 59u)], 1);
                        if (!m59) {
                            atomicAdd(&hist[aoff + H_REF_MQ + mapQ], 1);
                            atomicAdd(&hist[(rev ? H_REV_MQS : H_FWD_MQS) + mapQ], 1);
                        }
                    }
                }
            };

            const uint32_t g0 = rb & ~3u;
            const uint32_t key0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)abase);   // (for the scalar unit, like rb and re)
            uint4 w4n = make_uint4(0, 0, 0, 0), a4n = make_uint4(0, 0, 0, 0);
            uint32_t e4n = 0;
            auto fetch = [&](uint32_t i4) {
                if (i4 >= re) return;
                if (i4 + 3 < n_reads_tot) {
                    w4n = *reinterpret_cast<const uint4*>(p_rd + i4);
                    if (want_epos) e4n = *reinterpret_cast<const uint32_t*>(p_epos + i4);
                    if (INDEL) a4n = *reinterpret_cast<const uint4*>(p_aux + i4);
                } else {                                         // the last reads of the tile
                    uint32_t t4[4] = {0, 0, 0, 0}, x4[4] = {0, 0, 0, 0};
                    e4n = 0;
                    for (int j = 0; j < 4; ++j) if (i4 + j < n_reads_tot) {
                        t4[j] = p_rd[i4 + j];
                        if (want_epos) e4n |= (uint32_t)p_epos[i4 + j] << (8 * j);
                        if (INDEL) x4[j] = p_aux[i4 + j];
                    }
                    w4n = make_uint4(t4[0], t4[1], t4[2], t4[3]); a4n = make_uint4(x4[0], x4[1], x4[2], x4[3]);
                }
            };
            // A trip: the wavefront's 256 consecutive reads from `first` on, the lane's four from first + l4; the next trip
            // of the wavefront is 4 * WG reads on.  `first` and everything the trips are chosen by is wave-uniform.
            uint32_t l4 = 4u * (uint32_t)(tid & 63);
            uint32_t first = g0 + 256u * (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
            // A FULL trip has all its 256 reads inside [rb, re), and the loads for the trip behind it (reads past `re`, may be)
            // lie inside the tile's arrays: full_lo <= first <= full_hi.  It needs no byte mask, stores its keys with one
            // 8-byte store a lane, and loads without a guard, from a scalar base and a lane offset that stays the same.
            const bool fulls = re >= 1u * WG && n_reads_tot >= 5u * WG;
            const uint32_t full_lo = fulls ? rb : 0xffffffffu, full_hi = fulls ? min(re - 1u * WG, n_reads_tot - 5u * WG) : 0u;
            auto fetch_full = [&](uint32_t at, uint4 &w, uint4 &a, uint32_t &e) {
                // (the lane offset as a value of this trip: widened to 64 bits once, outside the loop, it is no longer seen to
                // be a 32-bit offset from a scalar base, and the address is formed by the lane)
                asm volatile("" : "+v"(l4)); uint32_t l16 = 4u * l4;
                w = load_global<u32x4>(p_rd + at, l16);
                if (want_epos) e = load_global<uint32_t>(p_epos + at, l4);
                if (INDEL) a = load_global<u32x4>(p_aux + at, l16);
            };
            fetch(first + l4);
            while (first < re) {
                if (first >= full_lo && first <= full_hi) {
                    do {
                        uint16_t *kq = s_key + (first - key0);
                        const uint4 w4 = w4n, a4 = a4n;
                        const uint32_t e4 = e4n;
                        uint32_t k01, k23;
                        fetch_full(first + 4u * WG, w4n, a4n, e4n);
                        quad(w4, a4, e4, 0xffffffffu, k01, k23);
                        *reinterpret_cast<uint2*>(kq + l4) = make_uint2(k01, k23);
                        first += 4u * WG;
                    } while (first <= full_hi);
                    continue;
                }
                // every other trip: a ragged end of the segment, the tile's last reads
                const uint32_t i4 = first + l4;
                const uint4 w4 = w4n, a4 = a4n;
                const uint32_t e4 = e4n;
                fetch(i4 + 4u * WG);                             // the next trip's loads fly while this one is worked on
                if (i4 < re) {
                    // the reads of [i4, i4 + 4) inside [rb, re): bytes lo .. hi-1 (i4 >= g0 = rb & ~3, so lo <= 3)
                    const uint32_t lo = rb > i4 ? rb - i4 : 0u, hi = min(re - i4, 4u);
                    const uint32_t vm4 = (0xffffffffu << (8 * lo)) & (hi == 4u ? 0xffffffffu : ~(0xffffffffu << (8 * hi)));
                    uint32_t k01, k23;
                    quad(w4, a4, e4, vm4, k01, k23);
                    uint16_t *kq = s_key + (first - key0) + l4;    // the lane's four keys
                    if (vm4 == 0xffffffffu) {                    // the four reads inside the segment: one 8-byte LDS store
                        *reinterpret_cast<uint2*>(kq) = make_uint2(k01, k23);
                    } else {                                     // a lane at a ragged end of the segment
                        const uint32_t kv[4] = { k01 & 0xffffu, k01 >> 16, k23 & 0xffffu, k23 >> 16 };
                        #pragma unroll
                        for (int u = 0; u < 4; ++u) if ((vm4 >> (8 * u)) & 1) kq[u] = (uint16_t)kv[u];
                    }
                }
                first += 4u * WG;
            }
            // ---- the segment's site totals ----
            // LDS mode: every lane adds its partial sums and counts to its own column of the slot's [value][pcol] table (no
            // conflicts inside a wave); the columns are added up once, when the workgroup is through (below).
            const uint32_t v[NPART] = { A.t_bq - A.d_bq, A.t_bq2 - A.d_bq2, A.d_bq, A.d_bq2, A.t_mq - A.d_mq, A.t_mq2 - A.d_mq2, A.d_mq, A.d_mq2,
                                        A.t_md - A.d_md, A.t_md2 - A.d_md2, A.d_md, A.d_md2, C.ori, C.mq0, C.m59, C.ref59, C.rev59 };
            if (LDS_HIST) {
                int col = tid & (pcol - 1);                      // (formed here, every segment: not a value kept alive through the rounds)
                asm volatile("" : "+v"(col));
                uint32_t *pt = s_part + (sg - site0) * (NPART * pcol) + col;
                #pragma unroll
                for (int j = 0; j < NPART; ++j) atomicAdd(&pt[j * pcol], v[j]);
            } else {
                // global mode (many sites per workgroup, i.e. very few samples): wave sums, one atomic per wave and value
                unsigned long long *tot = P.site_sums + (size_t)sg * SITE_NSUM;
                uint32_t x[NPART];
                #pragma unroll
                for (int j = 0; j < NPART; ++j) x[j] = wave_sum_u32(v[j]);
                if ((tid & 63) == 0) {
                    #pragma unroll
                    for (int j = 0; j < SITE_NSUM; ++j) if (x[j]) atomicAdd(&tot[j], (unsigned long long)x[j]);
                    const uint32_t m59 = x[SITE_NSUM], ref59 = x[SITE_NSUM + 1], rev59 = x[SITE_NSUM + 2];
                    if (ref59) atomicAdd(&hist[H_REF_MQ + 59], (int)ref59);
                    if (m59 - ref59) atomicAdd(&hist[H_ALT_MQ + 59], (int)(m59 - ref59));
                    if (m59 - rev59) atomicAdd(&hist[H_FWD_MQS + 59], (int)(m59 - rev59));
                    if (rev59) atomicAdd(&hist[H_REV_MQS + 59], (int)rev59);
                }
            }
        }
        __syncthreads();
        if (LDS_HIST) {
            // the columns of every partial sum: four lanes per value
            const int nslot = min(P.hist_slots, P.n_sites - site0), q4 = pcol >> 2;
            int i0 = tid;                                        // (formed here, every round, like the clearing loop's above)
            asm volatile("" : "+v"(i0));
            for (int i = i0; i < nslot * NPART * 4; i += WG) {
                const uint32_t *pt = s_part + (i >> 2) * pcol + (i & 3) * q4;
                unsigned long long x = 0;
                for (int k = 0; k < q4; ++k) x += pt[k];
                x += __shfl_xor(x, 1); x += __shfl_xor(x, 2);
                if ((i & 3) == 0 && x) {
                    const int vi = i >> 2, sl = vi / NPART, j = vi % NPART;
                    if (j < SITE_NSUM) s_tot[sl * SITE_NSUM + j] += x;
                    else {                                   // the mapQ 59 bins of the site's global histograms: all reads count as
                        const int c = (int)(uint32_t)x;      // ALT and forward, the REF and the reverse ones are moved over
                        int *g = P.hist + (long)(site0 + sl) * H_SIZE;
                        if (j == SITE_NSUM) { atomicAdd(&g[H_ALT_MQ + 59], c); atomicAdd(&g[H_FWD_MQS + 59], c); }
                        else if (j == SITE_NSUM + 1) { atomicAdd(&g[H_REF_MQ + 59], c); atomicAdd(&g[H_ALT_MQ + 59], -c); }
                        else { atomicAdd(&g[H_REV_MQS + 59], c); atomicAdd(&g[H_FWD_MQS + 59], -c); }
                    }
                }
            }
            __syncthreads();
        }

        // ================= phase B: one lane per cell =================
        uint16_t *kp_w = s_key + (part ? beg - abase : 0);       // the lane's keys
        const uint16_t *kp = kp_w;
        const int cnt_raw = part ? (int)(end - beg) : 0;
        // A cell with more than 255 usable reads.  bcf_call_glfgen counts every read (QS, ADF/ADR, anno[], SCR, the site's I16
        // sums and histograms: bam2bcf.c:203-252, all done by phase A or below over all keys); only errmod_cal cuts its input to
        // 255 (bam2bcf.c:256; htslib errmod.c draws them with hts_drand48, one generator for the whole process).
        // Here the cell's counts over ALL reads go to a WideRec (kernels.h), and the keys errmod_cal would not take are cleared
        // so that everything below -- which only feeds the likelihoods of such a cell -- sees 255 reads: the ones marked by
        // bcfgpu_errmod_plan (draw.hip: the draw replayed in mpileup's visit order), else the first 255, which is counted in
        // P.trunc (bcfgpu_truncated_cells: cells whose PLs may deviate from a reference run).
        if (__any(cnt_raw > BCFGPU_MAX_DEPTH)) {
            if (cnt_raw > BCFGPU_MAX_DEPTH) {
                int tw = tid;                                    // (the cell's index, formed here: see cellE below)
                asm volatile("" : "+v"(tw));
                const long cellW = cell0 + tw;
                uint32_t nus = 0;
                for (int i = 0; i < cnt_raw; ++i) nus += kp_w[i] != 0 ? 1u : 0u;
                const volatile unsigned long long *t = reinterpret_cast<const volatile unsigned long long*>(P.crp);
                uint64_t *qs64_p = reinterpret_cast<uint64_t*>(t[2]); uint32_t *misc_p = reinterpret_cast<uint32_t*>(t[6]);
                uint32_t mark = 0;
                if (nus > BCFGPU_MAX_DEPTH) {
                    uint32_t qs[4] = {0, 0, 0, 0}, af[4] = {0, 0, 0, 0}, ar[4] = {0, 0, 0, 0}, cn[4] = {0, 0, 0, 0}, sc = 0, acc = 0;
                    const bool all_diff = !INDEL && ref4c >= 4;
                    // which 255 feed the likelihoods: the ones bcfgpu_errmod_plan drew for this cell (draw.hip: its bitmap has
                    // exactly 255 of the cell's usable reads marked), else the first 255
                    bool planned = false;
                    if (P.draw_bits) {
                        uint32_t nm = 0;
                        for (int i = 0; i < cnt_raw; ++i) { const uint32_t ri = beg + (uint32_t)i; nm += (kp_w[i] != 0 && ((P.draw_bits[ri >> 5] >> (ri & 31)) & 1u)) ? 1u : 0u; }
                        planned = nm == BCFGPU_MAX_DEPTH;
                    }
                    for (int i = 0; i < cnt_raw; ++i) {
                        const uint32_t k = kp_w[i];
                        if (k == 0) continue;
                        const uint32_t rev = KEY_REV(k), q = KEY_Q(k), b = KEY_B(k);
                        const uint32_t dr = ((all_diff || !(k & KEY_PRIM)) ? 2u : 0u) | rev;     // anno[0<<2 | is_diff<<1 | is_rev]
                        #pragma unroll
                        for (uint32_t x = 0; x < 4; ++x) {
                            qs[x] += b == x ? q : 0u;
                            af[x] += (b == x && !rev) ? 1u : 0u; ar[x] += (b == x && rev) ? 1u : 0u;
                            cn[x] += dr == x ? 1u : 0u;
                        }
                        sc += KEY_SC(k);
                        bool stays = ++acc <= BCFGPU_MAX_DEPTH;
                        if (planned) { const uint32_t ri = beg + (uint32_t)i; stays = ((P.draw_bits[ri >> 5] >> (ri & 31)) & 1u) != 0; }
                        if (!stays) kp_w[i] = 0;
                    }
                    const uint32_t slot = atomicAdd(P.wide_ctr, 1u);
                    const uint32_t big = af[0] | af[1] | af[2] | af[3] | ar[0] | ar[1] | ar[2] | ar[3] | cn[0] | cn[1] | cn[2] | cn[3] | sc;
                    if (slot >= P.wide_cap || big > 0xffffu) atomicExch(P.err, BCFGPU_E_DEPTH);     // (16-bit count planes; the list is sized n_reads / 256)
                    else {
                        WideRec *w = reinterpret_cast<WideRec*>(t[7]) + slot;
                        #pragma unroll
                        for (int x = 0; x < 4; ++x) { w->qs[x] = qs[x]; w->ad[x] = af[x] | ar[x] << 16; }
                        w->cnt[0] = cn[0] | cn[1] << 16; w->cnt[1] = cn[2] | cn[3] << 16;
                        w->scr = sc; w->n = nus; w->cell = (uint32_t)cellW; w->pad[0] = w->pad[1] = w->pad[2] = 0;
                        qs64_p[cellW] = WIDE_QS_MARK | slot;      // where combine_kernel's frequency pass finds the record
                        mark = CR_WIDE;
                    }
                    if (!planned) atomicAdd(P.trunc, 1u);
                }
                misc_p[cellW] = mark;             // read back where the cell's planes are stored (below)
            }
        }
        // the soft-clipped reads, when SCR is asked for (mpileup's default leaves it out): a pass of its own
        uint32_t scr = 0;
        if (want_scr) for (int i = 0; i < cnt_raw; ++i) scr += KEY_SC((uint32_t)kp[i]);
        // pass 1: the quality mask of the primary base; the few other reads are gathered at the front of the slice
        uint64_t qmask = 0;          // qualities seen among the reads of the primary base
        uint32_t n_prim = 0;
        uint64_t qs64 = 0;           // QS[0..3], 16 bits each
        uint64_t ad64 = 0;           // ADF[0..3] | ADR[0..3]<<32, 8 bits each
        uint32_t n_b4 = 0;           // reads showing neither A, C, G nor T
        uint32_t o_rev = 0, n_other = 0;
        {
            uint32_t k_nx = kp[0];
            for (int i = 0; i < cnt_raw; ++i) {
                const uint32_t k = k_nx;
                k_nx = kp[i + 1];                               // one past the slice stays inside the key array's slack
                const uint32_t pb = k >> 11;                    // KEY_PRIM, the top bit of a key
                qmask |= (uint64_t)pb << KEY_Q(k);
                n_prim += pb;
                if (k - 1u < KEY_PRIM - 1u) {                   // rare: a read that is neither rejected (0) nor of the primary base
                    // swapped to position n_other <= i (behind the reader): the walks only count reads per (base, quality,
                    // strand), so the order inside a cell is free
                    const uint32_t t = kp_w[n_other], rev = KEY_REV(k), q = KEY_Q(k), b = KEY_B(k);
                    kp_w[n_other] = (uint16_t)k; kp_w[i] = (uint16_t)t;
                    ++n_other; o_rev += rev;
                    if (b < 4) { qs64 += (uint64_t)q << (16 * b); ad64 += 1ull << (8 * b + 32 * rev); }
                    else ++n_b4;
                }
            }
        }
        const uint32_t n = n_prim + n_other;                 // <= 255
        const bool dead_cell = n == 0;                       // nothing to walk (also the refused cells)
        const char *bbase = reinterpret_cast<const char*>(P.beta);
        const uint32_t brow = n << 3;

        // ---- errmod_cal: descending walk per base ----
        double bsum[5] = {0, 0, 0, 0, 0};
        uint32_t prim_rev = 0, qs_prim = 0;
        // (a) the primary base
        {
            const uint16_t *kpp = kp + n_other;               // primary-base keys and zeros (rejected reads)
            const PrimSrc psrc{kpp};
            const double bs = walk_runs(s_cnt, qmask, s_fk, bbase, P.pfx, tid, brow, psrc, dead_cell ? 0 : cnt_raw - (int)n_other, prim_rev, qs_prim);
            #pragma unroll
            for (int b = 0; b < 5; ++b) if (b == primary) bsum[b] = bs;
        }
        if (primary < 4) {
            qs64 += (uint64_t)qs_prim << (16 * primary);
            ad64 += (uint64_t)(n_prim - prim_rev) << (8 * primary) | (uint64_t)prim_rev << (8 * primary + 32);
        } else n_b4 += n_prim;
        // per-base counts c[0..4] (errmod_cal's aux.c)
        int c[5];
        #pragma unroll
        for (int b = 0; b < 4; ++b) c[b] = (int)((ad64 >> (8 * b)) & 0xff) + (int)((ad64 >> (8 * b + 32)) & 0xff);
        c[4] = (int)n_b4;
        // (b) the other bases present in the wave
        const bool any_other = __any(n_other > 0);
        if (any_other && __all(n_other <= 1)) {
            // No cell of the wavefront has two other reads (99 wavefronts in 100 of those that have any): the lane's other read
            // is kp[0], alone of its base -- the walk of that base is fk[0] * beta[q][0][n] added to +0, the expression of the
            // loop's "no cell shows a base twice" form below, without the loops over bases and keys.
            const bool one = n_other == 1 && !dead_cell;
            const uint32_t k = kp[0];
            const int b = (int)KEY_B(k);
            const uint32_t off1 = one ? (KEY_Q(k) << 19) + brow : brow;
            const double B1 = *reinterpret_cast<const double*>(bbase + off1);
            const double F1 = one ? s_fk[0] : s_fk[256];
            double bs = 0.;
            bs += F1 * B1;
            #pragma unroll
            for (int bb = 0; bb < 5; ++bb) if (one && bb == b) bsum[bb] = bs;
        } else if (any_other) {
            #pragma unroll 1
            for (int b = 0; b < 5; ++b) {
                int cb = b == 0 ? c[0] : b == 1 ? c[1] : b == 2 ? c[2] : b == 3 ? c[3] : c[4];
                if (b == primary || dead_cell) cb = 0;
                if (!__any(cb > 0)) continue;
                // key7 of the lane's i-th other read if it shows base b, else -1
                const BaseSrc src{kp, b};
                const int no = cb > 0 ? (int)n_other : 0;
                double bs;
                if (!__any(cb > 1)) {
                    // No cell of the wavefront has two reads of this base (sequencing errors: three wavefronts in four): a lane's walk
                    // would be its one read -- the first of its strand and of its base, fk[0] * beta[q][0][n] added to +0 -- without the
                    // slot counting and the run bookkeeping around it.
                    int key = -1;
                    for (int i = 0; __any(i < no); ++i) { const int k7 = i < no ? src(i) : -1; if (k7 >= 0) key = k7; }
                    const uint32_t off1 = key >= 0 ? ((uint32_t)(key >> 1) << 19) + brow : brow;
                    const double B1 = *reinterpret_cast<const double*>(bbase + off1);
                    const double F1 = key >= 0 ? s_fk[0] : s_fk[256];
                    bs = 0.;
                    bs += F1 * B1;
                } else {
                uint64_t qm = 0;
                for (int i = 0; i < no; ++i) { const int key = src(i); if (key >= 0) qm |= 1ull << (key >> 1); }
                uint32_t r_, q_;
                bs = walk_runs(s_cnt, qm, s_fk, bbase, P.pfx, tid, brow, src, no, r_, q_);
                }
                if (cb > 0) {
                    #pragma unroll
                    for (int bb = 0; bb < 5; ++bb) if (bb == b) bsum[bb] = bs;
                }
            }
        }
        const uint32_t n_rev = prim_rev + o_rev;

        // ---- epilogue of errmod_cal (m=5): float accumulators as in the reference ----
        uint32_t code = 0;
        // The planes' addresses are read here, from device memory, with loads the optimiser must leave in place: as kernel
        // arguments they are invariant over the staging rounds, the address of every (plane, cell) would be formed at the
        // top of the kernel and live in registers (or in scratch) through both phases.
        CallretPlanes cr;
        {
            const volatile unsigned long long *t = reinterpret_cast<const volatile unsigned long long*>(P.crp);
            cr.p15 = reinterpret_cast<float*>(t[0]); cr.pa = reinterpret_cast<float*>(t[1]);
            cr.qs64 = reinterpret_cast<uint64_t*>(t[2]); cr.adf = reinterpret_cast<uint32_t*>(t[3]);
            cr.adr = reinterpret_cast<uint32_t*>(t[4]); cr.cnt4 = reinterpret_cast<uint32_t*>(t[5]);
            cr.misc = reinterpret_cast<uint32_t*>(t[6]);
        }
        int te = tid;                                            // (the cell's index is formed here again: `cell` need not live
        asm volatile("" : "+v"(te));                             // through both phases for the stores below)
        const long cellE = cell0 + te;
        if (part) {
            const int nbases = (c[0] > 0) + (c[1] > 0) + (c[2] > 0) + (c[3] > 0) + (c[4] > 0);
            if (nbases <= 1) {
                // one base b (or no read at all): every sum over "the other bases" is bsum[b] or nothing, see CallretPlanes
                const int b = c[1] > 0 ? 1 : c[2] > 0 ? 2 : c[3] > 0 ? 3 : c[4] > 0 ? 4 : 0;
                double bsb = bsum[0];
                #pragma unroll
                for (int k = 1; k < 5; ++k) if (k == b) bsb = bsum[k];
                float A = n > 0 ? (float)((double)0.0f + bsb) : 0.0f;
                if (A < 0.0f) A = 0.0f;
                cr.pa[cellE] = A;
                code = (uint32_t)b;
            } else {
                code = CR_FULL;                                  // (its 15 likelihoods are formed below, a lane each)
            }
        }
        // A cell with reads of two or more bases (one cell in a hundred; every other wavefront holds one or two): the wavefront
        // takes them one after the other, the cell's sums and counts handed to every lane, and lane z < 15 forms likelihood
        // z = tri(j, k) -- errmod_cal's expressions (errmod.c: the float accumulators tmp1 / tmp3 over the bases other than j and
        // k in ascending order, lhet for j != k), "base i is left out" being a select on the lane's (j, k) around the same additions.
        if (const uint64_t fmask = __ballot(code == CR_FULL)) {
            int tl = tid;                                        // (the lane's genotype is formed here, every time: hoisted out of the
            asm volatile("" : "+v"(tl));                         // rounds it is three more values alive through both phases)
            const uint32_t lane = (uint32_t)tl & 63u, z = min(lane, 15u);
            const uint32_t j = (uint32_t)(GLF_TRI_J >> (4 * z)) & 7u, k = (uint32_t)(GLF_TRI_K >> (4 * z)) & 7u;
            // c[0..3] a byte each (forward + reverse strand: no sum passes n <= 255), c[4] | n << 8
            const uint32_t cpk = (uint32_t)ad64 + (uint32_t)(ad64 >> 32), c4n = n_b4 | n << 8;
            for (uint64_t fm = fmask; fm; fm &= fm - 1) {
                const int l = __builtin_ctzll(fm);                // the lane that owns the cell
                double bu[5];
                #pragma unroll
                for (int i = 0; i < 5; ++i) bu[i] = lane_f64(bsum[i], l);
                const uint32_t c03 = lane_u32(cpk, l), c4nu = lane_u32(c4n, l), nu = c4nu >> 8;
                const int cj = (int)perm(c4nu, c03, 0x0c0c0c00u | j), ck = (int)perm(c4nu, c03, 0x0c0c0c00u | k);     // byte 4: c[4]
                const bool het = j != k;
                float t1 = 0.0f;
                #pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const float tn = (float)((double)t1 + bu[i]);
                    t1 = ((uint32_t)i == j || (uint32_t)i == k) ? t1 : tn;
                }
                const int t2 = (int)nu - cj - (het ? ck : 0);      // the reads of the bases other than j and k: n is the sum of c[]
                float v = 0.0f;
                if (nu > 0) {
                    const double lh = -4.343 * P.lhet[het ? (cj + ck) << 8 | ck : 0];
                    const float h = t2 ? (float)(lh + (double)t1) : (float)lh;
                    v = het ? h : t2 ? t1 : 0.0f;
                }
                if (v < 0.0f) v = 0.0f;
                if (lane < 15u) cr.p15[(size_t)(cellE + (l - (int)lane)) * 16 + lane] = v;       // the cell's record: 15 likelihoods in 64 bytes
            }
        }
        if (part) {
            // anno[0..3]: ref/alt x fwd/rev counts.  "diff" reads are exactly the non-primary ones when the
            // reference base is A/C/G/T (or at indel sites); with an N reference every read is a diff read.
            const bool all_diff = (!INDEL && ref4c >= 4);
            const uint32_t n_fwd = n - n_rev;
            const uint32_t d_rev = all_diff ? n_rev : o_rev, d_fwd = all_diff ? n_fwd : n_other - o_rev;
            const uint32_t cnt4 = (n_fwd - d_fwd) | (n_rev - d_rev) << 8 | d_fwd << 16 | d_rev << 24;
            // (an over-deep cell: its mark and its WideRec index were left above; qs64 keeps the index, the packed counts below are
            // those of the 255 reads the likelihoods were made of -- their sum is the n of errmod_cal)
            uint32_t wm = 0;
            if (cnt_raw > BCFGPU_MAX_DEPTH) wm = *reinterpret_cast<volatile uint32_t*>(&cr.misc[cellE]) & CR_WIDE;
            if (!wm) cr.qs64[cellE] = qs64;
            cr.adf[cellE] = (uint32_t)ad64; cr.adr[cellE] = (uint32_t)(ad64 >> 32); cr.cnt4[cellE] = cnt4;
            cr.misc[cellE] = code | wm | (scr & 0xff) << 8;  // mq0 and ori_depth only feed site totals: site_sums[12..13]
            done = true;
        }
        if (nb == 0xffffffffu) break;
        base = nb;
        if (!DEEP && !done && deep && beg == base) s_skip = end; // a listed cell at the head of the line: the rounds step over its reads
        __syncthreads();                                         // the slot counters are phase A's partial sums again
        if (!DEEP) {
            const uint32_t sk = s_skip, pend = PACKED ? s_pend : 0u;
            if (sk) { if (deep && beg == base) done = true; base = sk; }
            __syncthreads();                                     // (s_skip is cleared at the top of the round)
            if (PACKED) {
                // Another round: the reads it can add to a bin are at most its window.  Could a half pass HP_MAX with them, the
                // copy is added to the global histograms and cleared first (uniform: every lane has read the same s_pend before
                // the barrier above; the cleared dwords are seen after the barrier at the top of the round).
                const uint32_t win = min((base & ~3u) + (uint32_t)cap, span_end) - base, p = pend + win;
                const bool fl = p > HP_MAX;
                if (tid == 0) s_pend = fl ? win : p;
                if (fl) flush_packed(true);
            }
        }
    }

    // ---- flush the workgroup's histograms and site totals ----
    if (LDS_HIST) {
        __syncthreads();
        int nsite = P.n_sites;                                   // (formed here: the same count from the kernel's top is one more value
        asm volatile("" : "+s"(nsite));                          // alive through every round)
        const int nslot = min(P.hist_slots, nsite - site0);
        if (PACKED) flush_packed(false);
        else {                                                   // a deep cell's site: plain counters in the global layout
            int *g = P.hist + (long)site0 * H_SIZE;
            for (int i = tid; i < H_SIZE; i += WG) { const int v = s_hist[i]; if (v) atomicAdd(&g[i], v); }
        }
        for (int i = tid; i < nslot * SITE_NSUM; i += WG) {
            const unsigned long long v = s_tot[i];
            if (v) atomicAdd(&P.site_sums[(size_t)site0 * SITE_NSUM + i], v);
        }
    }
}

// The prefix table of walk_runs() (kernels.h), stored [q][n][r][f]: one lane per (q, n, r); the lanes of a wavefront differ in
// n (the thread index is decoded with n fastest), so that its loads of beta[q][k][n] are one row.  The
// lane forms the sum of its r reverse-strand reads, then stores it as f = 0 and after every forward-strand read it adds -- the
// walk's order, a multiply and an add per read (-ffp-contract=off), so an entry has the bits the walk reaches read by read.
// beta is read at k = r + f - 1 <= 2 * GLF_PFX_S - 3; entries with r + f > n are never looked up.
static_assert(2 * GLF_PFX_S - 3 < 256 && GLF_PFX_N <= 256 && GLF_PFX_S <= 256, "the prefix table stays inside fk[256] and beta[64][256][256]");
__global__ __launch_bounds__(WG) void glfgen_prefix_kernel(const double *fk, const double *beta, double *pfx)
{
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= 64u * GLF_PFX_S * GLF_PFX_N) return;
    const uint32_t n = i % GLF_PFX_N, r = i / GLF_PFX_N % GLF_PFX_S, q = i / (GLF_PFX_N * GLF_PFX_S);
    const double *b = beta + ((size_t)q << 16 | n);                 // beta[q][k][n] = b[k << 8]
    double *t = pfx + (((size_t)q * GLF_PFX_N + n) * GLF_PFX_S + r) * GLF_PFX_S;
    double bs = 0;
    for (uint32_t u = 0; u < r; ++u) bs += fk[u] * b[u << 8];
    t[0] = bs;
    for (uint32_t u = 0; u + 1 < (uint32_t)GLF_PFX_S; ++u) { bs += fk[u] * b[(r + u) << 8]; t[u + 1] = bs; }
}

void launch_glfgen_prefix(const double *fk, const double *beta, double *pfx, hipStream_t s)
{
    hipLaunchKernelGGL(glfgen_prefix_kernel, dim3(64 * GLF_PFX_S * GLF_PFX_N / WG), dim3(WG), 0, s, fk, beta, pfx);
}

size_t glfgen_lds_bytes(int cap, int hist_slots)
{
    return LDS_HIST_OFF + (size_t)hist_slots * (HP_SIZE * sizeof(int) + SITE_NSUM * 8) + ((size_t)cap + 8) * 2;
}

template <bool INDEL, bool LDS_HIST>
static void launch_one(const GlfgenParams &p, hipStream_t s, int grid, size_t lds)
{
    if (lds > 48 * 1024)    // per launch, on the device the caller has bound: no process-wide state
        hipFuncSetAttribute(reinterpret_cast<const void*>(glfgen_kernel<INDEL, LDS_HIST, false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((glfgen_kernel<INDEL, LDS_HIST, false>), dim3(grid), dim3(WG), lds, s, p);
    // the cells the launch above listed (none, as a rule: the workgroups leave at once); no key window in LDS
    if (p.deep_cap) hipLaunchKernelGGL((glfgen_kernel<INDEL, LDS_HIST, true>), dim3(p.deep_cap), dim3(WG), glfgen_lds_bytes(0, p.hist_slots), s, p);
}

void launch_glfgen(const GlfgenParams &p, hipStream_t s)
{
    const long ncells = (long)p.n_sites * p.n_smpl;
    if (ncells == 0) return;
    const int grid = (int)((ncells + WG - 1) / WG);
    const size_t lds = glfgen_lds_bytes(p.lds_cap, p.hist_slots);
    if (p.is_indel) { if (p.hist_slots) launch_one<true, true>(p, s, grid, lds); else launch_one<true, false>(p, s, grid, lds); }
    else            { if (p.hist_slots) launch_one<false, true>(p, s, grid, lds); else launch_one<false, false>(p, s, grid, lds); }
}

}  // namespace bcfgpu
