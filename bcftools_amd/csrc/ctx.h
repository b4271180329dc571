// ctx.h -- the context's internal interface, for the stages in their own translation units: the workspace slots and the
// accessors of bcfgpu_ctx.  Defined in api.hip, except the read pool's functions (pool.hip), scan_exclusive and enc_offsets
// (gather.hip) and bcfgpu_internal_gap_core (gap_prep.hip).  C++ linkage: none of it is part of the C-ABI of include/bcfgpu.h.
#pragma once
#include <thread>
#include <vector>
#include "kernels.h"

namespace bcfgpu {

// ---- the context's grow-only device workspaces (bcfgpu_internal_ws) ----
// One name per use; the prefix after WS_ names the entry point that uses it.  Names with the same value are one buffer, and
// each of their users takes it as scratch for one call (the work a call queues on it is ordered on the context's stream).
// "Kept" marks the slots whose contents a later entry point reads: they are listed in WS_KEPT below, and no other use may
// share their numbers (tests/test_ctx_slots.py checks both against this enum).
enum WsSlot : int {
    // the uploaded view of a bcfgpu_reads (pool_view_upload, the PoolSlots set POOL_VIEW below): scratch for one call of
    // bcfgpu_baq, bcfgpu_cap_mapq, bcfgpu_overlap_tweak or bcfgpu_gap_prep; bcfgpu_gap_prep_tile forms its per-read arrays and
    // uploads the caller's ZQ bytes there
    WS_VIEW_R_MAPQ = 38, WS_VIEW_R_POS = 40, WS_VIEW_R_LQ = 41, WS_VIEW_R_FLAG = 42, WS_VIEW_R_NCIG = 43, WS_VIEW_R_CIG_OFF = 44,
    WS_VIEW_R_SEQ_OFF = 45, WS_VIEW_CIG = 46, WS_VIEW_SEQ16 = 47, WS_VIEW_QUAL = 48, WS_VIEW_ZQ = 49, WS_VIEW_HAS_ZQ = 50,
    // bcfgpu_baq: what baq_core writes for it (bcfgpu_pool_baq hands the core the pool's kept slots instead): scratch for one call
    WS_BAQ_QUAL_OUT = 14, WS_BAQ_ZQ_OUT = 15, WS_BAQ_HAS_ZQ = 8,

    // the read pool (pool.hip pool_upload_impl).  Kept: DevPool, read by the pool stages below and bcfgpu_pool_pileup
    WS_POOL_CIG = 27, WS_POOL_SEQ16 = 28, WS_POOL_QUAL = 29,
    WS_POOL_R_POS = 104, WS_POOL_R_LQ = 105, WS_POOL_R_FLAG = 106, WS_POOL_R_NCIG = 107, WS_POOL_R_CIG_OFF = 108,
    WS_POOL_R_SEQ_OFF = 109, WS_POOL_R_MAPQ = 110,
    //   the upload's packed inputs: scratch for one call
    WS_POOL_SEQ4 = 111, WS_POOL_QUAL4 = 112, WS_POOL_RECS = 128, WS_POOL_SCAN_TMP = 129,
    WS_POOL_KEEP = 114,                 // kept: DevPool::keep (bcfgpu_pool_keep), read by bcfgpu_pool_pileup
    WS_POOL_EXTENT = 122,               // bcfgpu_internal_pool_extent (of the pool or of a view): scratch for one call
    //   the second set of the pool's arrays.  Kept: the pool bcfgpu_pool_stage brings up lands in the set the context's pool
    //   is not in, and bcfgpu_pool_adopt makes that set the pool's (PoolStage::set says which one DevPool points into)
    WS_POOL_B_CIG = 154, WS_POOL_B_SEQ16 = 155, WS_POOL_B_QUAL = 156, WS_POOL_B_R_POS = 157, WS_POOL_B_R_LQ = 158,
    WS_POOL_B_R_FLAG = 159, WS_POOL_B_R_NCIG = 160, WS_POOL_B_R_CIG_OFF = 161, WS_POOL_B_R_SEQ_OFF = 162, WS_POOL_B_R_MAPQ = 163,
    //   a staged pool's packed inputs.  Kept from bcfgpu_pool_stage to bcfgpu_pool_adopt, which expands them
    WS_POOL_STAGE_SEQ4 = 164, WS_POOL_STAGE_QUAL4 = 165, WS_POOL_STAGE_RECS = 166,
    // baq_core (bcfgpu_pool_baq and, on a view, bcfgpu_baq): scratch for one call
    WS_PBAQ_JOBS0 = 0, WS_PBAQ_JOBS1 = 3, WS_PBAQ_JOBS2 = 127, WS_PBAQ_JOBS3 = 135, WS_PBAQ_JOBS2_SORTED = 128,
    WS_PBAQ_COUNTS = 115, WS_PBAQ_RET = 116, WS_PBAQ_STATE = 11, WS_PBAQ_Q = 12, WS_PBAQ_TMP = 13,
    WS_PBAQ_REF = 121, WS_PBAQ_REF4 = 7,
    //   the matrices of band class c: F, S and W (W of the LDS-row classes 2 and 3: their second matrix)
    WS_PBAQ_F0 = 4, WS_PBAQ_S0 = 2, WS_PBAQ_W0 = 5, WS_PBAQ_F1 = 144, WS_PBAQ_S1 = 145, WS_PBAQ_W1 = 146,
    WS_PBAQ_F2 = 147, WS_PBAQ_S2 = 148, WS_PBAQ_W2 = 1, WS_PBAQ_F3 = 149, WS_PBAQ_S3 = 150, WS_PBAQ_W3 = 151,
    //   kept: the pool's new qualities (DevPool::qual; the call writes to the one of the two it is not in), ZQ and which reads
    //   have it (DevPool::zq, r_has_zq), read by the pool stages after it, bcfgpu_pool_download and bcfgpu_gap_prep_tile
    WS_PBAQ_QUAL_A = 118, WS_PBAQ_QUAL_B = 119, WS_PBAQ_ZQ = 120, WS_PBAQ_HAS_ZQ = 117,
    // overlap_core, cap_core (the pool forms and, on a view, bcfgpu_overlap_tweak / bcfgpu_cap_mapq): scratch for one call
    WS_POVL_PAIR_A = 123, WS_POVL_PAIR_B = 124,
    WS_PCAPQ_REF = 125, WS_PCAPQ_OUT = 126,

    // bcfgpu_pool_pileup.  Kept: the SNP tile, read by bcfgpu_mpileup / bcfgpu_pipeline / bcfgpu_errmod_plan on it, and
    // through PileupParams by bcfgpu_pileup_entries, bcfgpu_pileup_indel_tile and bcfgpu_gap_prep_tile
    WS_PLP_REF16 = 16, WS_PLP_SMPL_OFF = 17, WS_PLP_S_POS = 18, WS_PLP_META = 19, WS_PLP_S_READ = 20,
    WS_PLP_CNT = 30, WS_PLP_RECS = 31,
    //   scratch for one call (the scan's temporary storage is done with before the records go to its buffer)
    WS_PLP_SCAN_TMP = 31, WS_PLP_TOTAL = 34, WS_PLP_STATUS = 113, WS_PLP_COL_COUNTS = 134,
    // bcfgpu_pileup_entries: scratch for one call
    WS_ENT_COLS = 21, WS_ENT_SEL = 22, WS_ENT_SCAN_TMP = 23, WS_ENT_OUT = 24,
    // bcfgpu_pileup_indel_tile and bcfgpu_gap_prep_tile.  Kept: the indel tile each returns, read by bcfgpu_mpileup /
    // bcfgpu_errmod_plan on it; each call has slots of its own, so that its tile stays valid through the other call
    WS_ITILE_SEL = 25, WS_ITILE_RECS = 26,
    WS_ITILE_COLS = 21, WS_ITILE_SCAN_TMP = 23,                                // scratch for one call
    WS_GTILE_LIVE_SEL = 131, WS_GTILE_RECS = 152,
    //   scratch for one call
    WS_GTILE_COLS = 21, WS_GTILE_N_KEPT = 143, WS_GTILE_SEL = 153, WS_GTILE_SCAN_TMP = 23, WS_GTILE_ENT = 24, WS_GTILE_LIVE = 130,

    // bcfgpu_gap_prep and bcfgpu_gap_prep_tile: scratch for one call.  The inputs beside the reads (the view above) as
    // bcfgpu_gap_prep uploads them (those bcfgpu_gap_prep_tile forms or uploads itself: the positions, the reference slice, p->aux)
    WS_GAP_POS = 51, WS_GAP_SMPL_OFF = 52,
    WS_GAP_P_READ = 53, WS_GAP_P_QPOS = 54, WS_GAP_P_INDEL = 55, WS_GAP_REF = 64, WS_GAP_AUX = 67,
    //   bcfgpu_internal_gap_core
    WS_GAP_INSCNT = 56, WS_GAP_INSCNS = 57, WS_GAP_REF2 = 58, WS_GAP_SCORE1 = 59, WS_GAP_SCORE2 = 60, WS_GAP_WIDE = 61,
    WS_GAP_OUT_INSCNS = 62, WS_GAP_WIDE_ROWS = 63, WS_GAP_SITES = 65, WS_GAP_READ_INFO = 66, WS_GAP_SMALL = 68, WS_GAP_ENT = 69,
    WS_GAP_QPACK = 70, WS_GAP_PJOB = 71, WS_GAP_KEY_IN = 72, WS_GAP_VAL_IN = 73, WS_GAP_KEY_SORTED = 74, WS_GAP_VAL_SORTED = 75,
    WS_GAP_LIST2 = 76, WS_GAP_SORT_TMP = 77, WS_GAP_QUEUE = 78, WS_GAP_SUMQ = 79, WS_GAP_OTYPE = 80, WS_GAP_EMT = 133,

    // bcfgpu_gvcf_blocks, bcfgpu_compact_calls[_async]: scratch for one call
    WS_GVCF_SCAN = 32, WS_GVCF_SCAN_TMP = 33,
    WS_COMPACT_SIZE = 35, WS_COMPACT_SCAN_TMP = 36, WS_COMPACT_COUNTS = 37,
    // the device codecs of the records' per-sample bytes (bcfcodec.h): scratch for one call.  The encoders' size passes
    // (enc_offsets) share the scan's temporary storage: each entry synchronises the context's stream before it returns
    WS_COMPACT_ENC_SCAN_TMP = 167,
    // bcfgpu_mplp_encode_bcf (bcfenc.hip): the keys' integer types per site
    WS_COMPACT_BCF_TYPES = 168,
    // bcfgpu_call_decode_bcf (bcfdec.hip): the uploaded copies of the records' vectors and of the sample map
    WS_COMPACT_BCFDEC_VEC = 169, WS_COMPACT_BCFDEC_COL = 170,
    // bcfgpu_call_encode_bcf (bcfcallenc.hip): one packed word a site (the three keys' integer types, GT's and PL's widths)
    WS_COMPACT_BCFCALL_WORD = 171,
    // bcfgpu_call_remap_bcf (bcfkeys.hip): the uploaded copies of the key jobs and of the sample map, one packed word a job (the
    // block's integer type and width)
    WS_COMPACT_BCFKEY_JOBS = 172, WS_COMPACT_BCFKEY_COL = 173, WS_COMPACT_BCFKEY_WORD = 174,
    // bcfgpu_call_encode_vcf (vcfcallenc.hip): the uploaded copies of the fields, of each site's first field and of the sample map
    WS_COMPACT_CALLVCF_FIELDS = 175, WS_COMPACT_CALLVCF_FIRST = 176, WS_COMPACT_CALLVCF_COL = 177,
    // bcfgpu_call_decode_vcf (vcfdec.hip): the uploaded copies of the records' runs and of the sample map, the offsets of the columns
    // of one chunk of sites (at most BCFGPU_VCFDEC_START_BYTES, or one site's), the two error words
    WS_COMPACT_VCFDEC_VEC = 178, WS_COMPACT_VCFDEC_COL = 179, WS_COMPACT_VCFDEC_START = 180, WS_COMPACT_VCFDEC_ERR = 181,
    // bcfgpu_call_rewrite_vcf (vcfcallrw.hip): the uploaded copies of the records' runs (as the indexing kernel reads them), of the
    // records and of the sample map, the offsets of the columns of one chunk of sites (bounded as bcfgpu_call_decode_vcf's), the error word
    WS_COMPACT_VCFRW_VEC = 182, WS_COMPACT_VCFRW_REC = 183, WS_COMPACT_VCFRW_COL = 184, WS_COMPACT_VCFRW_START = 185, WS_COMPACT_VCFRW_ERR = 186,
    // bcfgpu_call_parse_keys_vcf (vcfkeys.hip): the uploaded copies of the key jobs (each with its run's place among the indexed runs)
    // and of the sample map, one packed word a job (the block's integer type and width), one status byte a job, the runs of the sites
    // that have a job with a record (as the indexing kernel reads them), the offsets of the columns of one chunk of them (bounded as
    // bcfgpu_call_decode_vcf's), the error word
    WS_COMPACT_VCFKEY_JOBS = 187, WS_COMPACT_VCFKEY_COL = 188, WS_COMPACT_VCFKEY_WORD = 189, WS_COMPACT_VCFKEY_STATUS = 190,
    WS_COMPACT_VCFKEY_RUNS = 191, WS_COMPACT_VCFKEY_START = 192, WS_COMPACT_VCFKEY_ERR = 193,
    // bcfgpu_call_constrain (calsmap.hip): the uploaded copy of the sites' descriptors
    WS_COMPACT_CALS_SITE = 194,

    // bcfgpu_errmod_plan[_visit].  Kept: DrawState::bits, read by the next bcfgpu_mpileup / bcfgpu_pipeline on each tile
    WS_DRAW_BITS_SNP = 136, WS_DRAW_BITS_INDEL = 137,
    //   scratch for one call
    WS_DRAW_VISIT = 132, WS_DRAW_ENT = 138, WS_DRAW_CTR = 139, WS_DRAW_COLS = 140, WS_DRAW_IDX_OFF = 141, WS_DRAW_IDX = 142,

    WS_COUNT = WS_COMPACT_CALS_SITE + 1     // one past the highest slot
};

// the kept slots (see above): what each holds stays valid from the call that writes it until a call include/bcfgpu.h names
constexpr WsSlot WS_KEPT[] = {
    WS_POOL_CIG, WS_POOL_SEQ16, WS_POOL_QUAL, WS_POOL_R_POS, WS_POOL_R_LQ, WS_POOL_R_FLAG, WS_POOL_R_NCIG, WS_POOL_R_CIG_OFF,
    WS_POOL_R_SEQ_OFF, WS_POOL_R_MAPQ, WS_POOL_KEEP,
    WS_POOL_B_CIG, WS_POOL_B_SEQ16, WS_POOL_B_QUAL, WS_POOL_B_R_POS, WS_POOL_B_R_LQ, WS_POOL_B_R_FLAG, WS_POOL_B_R_NCIG,
    WS_POOL_B_R_CIG_OFF, WS_POOL_B_R_SEQ_OFF, WS_POOL_B_R_MAPQ, WS_POOL_STAGE_SEQ4, WS_POOL_STAGE_QUAL4, WS_POOL_STAGE_RECS,
    WS_PBAQ_QUAL_A, WS_PBAQ_QUAL_B, WS_PBAQ_ZQ, WS_PBAQ_HAS_ZQ,
    WS_PLP_REF16, WS_PLP_SMPL_OFF, WS_PLP_S_POS, WS_PLP_META, WS_PLP_S_READ, WS_PLP_CNT, WS_PLP_RECS,
    WS_ITILE_SEL, WS_ITILE_RECS, WS_GTILE_LIVE_SEL, WS_GTILE_RECS,
    WS_DRAW_BITS_SNP, WS_DRAW_BITS_INDEL,
};

// ---- the context's grow-only pinned host buffers (bcfgpu_internal_pinned): each is scratch for one call ----
enum PinnedSlot : int {
    PIN_GAP_SMALL = 0,                  // bcfgpu_internal_gap_core: the totals and per-site results
    PIN_COMPACT_COUNTS = 1,             // bcfgpu_compact_counts
    PIN_GTILE_KEPT = 2,                 // bcfgpu_gap_prep_tile: the columns that go on
    PIN_PLP_COL_COUNTS = 3,             // bcfgpu_pool_pileup: col_n / col_indel
    PIN_PBAQ_REF = 6,                   // bcfgpu_pool_baq: the reference slice (the call returns with its copy in flight)
    PIN_ENC_TOTAL = 7,                  // enc_offsets: the size of all blocks of an encoder entry (each synchronises before it returns)
    PIN_VCFDEC_ERR = 8,                 // bcfgpu_call_decode_vcf: the error words of its two passes (it synchronises before it reads them)
    PIN_VCFRW_ERR = 9,                  // bcfgpu_call_rewrite_vcf: the error word of its indexing pass (it synchronises before it reads it)
    PIN_VCFKEY_ERR = 10,                // bcfgpu_call_parse_keys_vcf: the error word of its indexing pass (it synchronises before it reads it)
    PINNED_COUNT = PIN_VCFKEY_ERR + 1       // one past the highest slot
};

// workspace / pinned host buffer `slot` of at least `bytes` (contents undefined); nullptr when the allocation fails
void *bcfgpu_internal_ws(bcfgpu_ctx *c, WsSlot slot, size_t bytes);
void *bcfgpu_internal_pinned(bcfgpu_ctx *c, PinnedSlot slot, size_t bytes);
// workspace `slot` of at least bytes + slack, the copy of `bytes` from host `src` queued on `stream`; nullptr on failure
void *ws_upload(bcfgpu_ctx *c, WsSlot slot, const void *src, size_t bytes, size_t slack, hipStream_t stream);

// bind the context's device, hand out its stream and the qual2prob table (either may be NULL); 0 on success
int bcfgpu_internal_device(bcfgpu_ctx *c, hipStream_t *stream, const float **q2p);
// the side streams (fork / join around independent launches), created on first use; 0 on success
int bcfgpu_internal_side(bcfgpu_ctx *c, hipStream_t **streams, hipEvent_t **events);
int bcfgpu_internal_n_cu(const bcfgpu_ctx *c);
const bcfgpu_cfg *bcfgpu_internal_cfg(const bcfgpu_ctx *c);
bcfgpu_gap_stats *bcfgpu_internal_gap_stats(bcfgpu_ctx *c);
DrawState *bcfgpu_internal_draw_state(bcfgpu_ctx *c);
DevPool *bcfgpu_internal_pool_state(bcfgpu_ctx *c);             // the read pool bcfgpu_pool_upload / bcfgpu_pool_adopt left in HBM
PileupParams *bcfgpu_internal_pileup_state(bcfgpu_ctx *c);      // the parameters of the last bcfgpu_pool_pileup
// The read pool's generation: every pool bcfgpu_pool_upload / bcfgpu_pool_adopt / bcfgpu_pileup[_packed] puts in place of the
// last is a new one.
// bcfgpu_internal_pool_replaced: the context's pool is about to be replaced (the old one's arrays are gone from here on).
// bcfgpu_internal_pileup_built: P is the new pileup, built from the context's pool as it is now (P.cnt = nullptr: none).
// bcfgpu_internal_pileup_pool_gone: the pool the last pileup was built from is no longer in the workspace -- the calls that
// read the pool through PileupParams must refuse then.
void bcfgpu_internal_pool_replaced(bcfgpu_ctx *c);
void bcfgpu_internal_pileup_built(bcfgpu_ctx *c, const PileupParams &P);
bool bcfgpu_internal_pileup_pool_gone(const bcfgpu_ctx *c);
// The staged read pool (bcfgpu_pool_stage / bcfgpu_pool_adopt, pool.hip): the pool has two sets of its kept slots, the
// context's pool in one and the pool a stage brings up in the other; adopting is a change of roles.
struct PoolStage {
    int set = 0;                        // the set DevPool points into: 0 = WS_POOL_*, 1 = WS_POOL_B_*
    int pending = 0;                    // a staged pool waits for bcfgpu_pool_adopt
    int freed_valid = 0;                // `freed` has been recorded
    hipStream_t copy = nullptr;         // the copy stream
    hipEvent_t copied = nullptr;        // on `copy`, behind the staged pool's host-to-device copies
    hipEvent_t freed = nullptr;         // on the context's stream at the last adopt, behind every reader of the set (and of the
                                        // staging slots) the next stage writes to
    DevPool D{};                        // the staged pool: its arrays in the other set (the packed forms': still to be formed)
    const bcfgpu_read12 *d_rec = nullptr;                   // its packed inputs in HBM (NULL: not that form) and how to read them
    const uint8_t *d_seq4 = nullptr, *d_qual4 = nullptr;
    unsigned long long pal[2] = {0, 0};
    int qual_bits = 0;
};
// the context's PoolStage; with_stream: its stream and events are created on first use, nullptr when that fails
PoolStage *bcfgpu_internal_pool_stage(bcfgpu_ctx *c, bool with_stream);
// The tile whose read records start workspace `recs` is about to be rebuilt: a draw plan made for it (DrawState::rd, matched by
// that address) is dropped, so that the new tile in the same buffer does not take it for its own.
void bcfgpu_internal_drop_plan(bcfgpu_ctx *c, WsSlot recs);
int bcfgpu_set_error(int code, const char *what);               // bcfgpu_last_error() becomes `what`; returns `code`
int bcfgpu_set_error(int code, const char *name, const char *what);     // ... becomes "`name`: `what`"
// a HIP call of an entry point: on an error, BCFGPU_E_HIP with the call's text, and the entry returns
#define BCFGPU_CHK(call) do { if ((call) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, #call); } while (0)
// d[0 .. n) becomes its exclusive sum, queued on st; the scan's temporary storage is workspace `slot`.  Returns 0, BCFGPU_E_HIP or
// BCFGPU_E_NOMEM (no error text is set).  The one instance of the device-wide exclusive scan in the library (gather.hip), for the
// element types in use: uint32_t / int32_t counts and 64-bit sizes.
template <class T> int scan_exclusive(bcfgpu_ctx *ctx, hipStream_t st, WsSlot slot, T *d, int n);

// ---- a bcfgpu_reads in HBM (pool.hip) ----
// One slot per array.  The context's pool lies in one of two sets of kept slots (POOL_SET, pool.hip); the host-pointer forms of
// the read stages upload their reads to POOL_VIEW, scratch for one call, and run the pool forms' cores on that view.
struct PoolSlots { WsSlot cig, seq16, qual, r_pos, r_lq, r_flag, r_ncig, r_cig_off, r_seq_off, r_mapq, zq, r_has_zq; };
constexpr PoolSlots POOL_VIEW = {WS_VIEW_CIG, WS_VIEW_SEQ16, WS_VIEW_QUAL, WS_VIEW_R_POS, WS_VIEW_R_LQ, WS_VIEW_R_FLAG, WS_VIEW_R_NCIG,
                                 WS_VIEW_R_CIG_OFF, WS_VIEW_R_SEQ_OFF, WS_VIEW_R_MAPQ, WS_VIEW_ZQ, WS_VIEW_HAS_ZQ};
// the arrays only some stages read: they go up when the caller asks for them, and may be NULL otherwise
enum : unsigned { READS_LQ = 1, READS_FLAG = 2, READS_MAPQ = 4, READS_ZQ = 8 };
// The arrays of `rd` (and r_mapq), as they are, to the slots `ps`, the copies queued on `stream`: the extents of the pools (the
// caller hands over pointers, not lengths), then *D = their description, valid = 0 (it is not the context's pool).  r_pos, r_ncig,
// r_cig_off, r_seq_off, cig, seq16 and qual always go up; r_lq (the host reads it in any case, for the extents), r_flag, r_mapq and
// zq / r_has_zq (those two: when `rd` has both) as `want` says, D's pointer NULL otherwise.  Errors are set as "`who`: ...".
int pool_view_upload(const char *who, bcfgpu_ctx *ctx, const bcfgpu_reads *rd, const uint8_t *r_mapq, unsigned want,
                     const PoolSlots &ps, hipStream_t stream, DevPool *D);
// [lowest start, highest end) of D's reads, kept in D once computed
int bcfgpu_internal_pool_extent(bcfgpu_ctx *ctx, DevPool &D, int *lo, int *hi);
// bcfgpu_pool_upload without its wait: `rd` / `pk` become the context's read pool, copies and kernels queued on the context's stream
// (bcfgpu_pileup[_packed] go on to the pileup and wait there, with the counts)
int pool_upload_impl(const char *who, bcfgpu_ctx *ctx, const bcfgpu_reads *rd, const bcfgpu_packed *pk, const uint8_t *r_mapq);
// host threads for a pass over n reads (at most 16, BCFGPU_HOST_THREADS), and fn(t) on each of them
int host_threads(int n);
template <class F> void on_threads(int nthr, F &&fn)
{
    std::vector<std::thread> thr;
    for (int t = 1; t < nthr; ++t) thr.emplace_back(fn, t);
    fn(0);
    for (auto &th : thr) th.join();
}
// The size pass of an encoder entry `name` behind its size kernel (gather.hip): d_off[0 .. n_off) holds the blocks' sizes and a
// last 0 and becomes their exclusive sum, the offsets; *n_bytes = their total, d_off[n_off - 1].  The stream is synchronised.
// n_off == 1 (nothing to encode, no size kernel): the one offset is set to 0.  Returns 0 -- the caller goes on to its write
// kernel unless *n_bytes is 0 --, or the entry's error: BCFGPU_E_RANGE when the total is above cap_bytes (nothing is written, the
// caller learns the size and may come back with a larger buffer).  Takes WS_COMPACT_ENC_SCAN_TMP and PIN_ENC_TOTAL.
int enc_offsets(bcfgpu_ctx *ctx, hipStream_t st, const char *name, uint64_t *d_off, int n_off, uint64_t cap_bytes, uint64_t *n_bytes);
// bcf_call_gap_prep on inputs already in HBM (gap_prep.hip)
int bcfgpu_internal_gap_core(bcfgpu_ctx *ctx, const GapIn &g, size_t n_ent, uint32_t *d_aux, const bcfgpu_indel_out *out, int inscns_cap);

}  // namespace bcfgpu
