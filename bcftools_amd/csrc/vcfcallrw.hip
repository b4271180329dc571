// vcfcallrw.hip -- the sample columns of a call record as VCF text, rewritten on the device from the input record's own text: what the
// text route does per written record of VCF text input on one host thread -- the columns split at tabs, every column at ':', every
// Number=R field at ',', and all of it printed again around GT, the trimmed PL and GQ (write_record, print_sample_text, print_gt and
// print_numberR of host/bcfgpu_call.c; vcf_format of htslib vcf.c behind mcall.c:1158-1265, :1583, :1618-1623).  vcfcallenc.hip with
// the input as text: a pass-through field is a token of the input column, copied as the bytes it is -- an integer, a Float or a String
// alike --, so no key sends a record back to the host for its type; only a Number=R token of a record that lost alleles is cut at ','
// and put together again in the alleles' new order.
//
//   vcfdec_index_kernel  (vcfdec.hip, launch_vcfdec_index) the offsets of every column's tab inside its record's run, and the check
//                        that the run is n_smpl_in columns
//   callrw_size_kernel   one workgroup a site, a lane a called sample: the length of every sample's text from its column where it
//                        lies in global memory, summed to the site's size
//   enc_offsets          the sites' offsets (the device scan, gather.hip)
//   callrw_write_kernel  one workgroup a site, a lane a called sample, in rounds cut by bytes on both sides.  Without a sample map the
//                        columns of the round's samples are one span of the run: it comes into the input stage by line_load, the
//                        lanes find their texts' lengths there, the lengths' exclusive scan places every text in the output stage,
//                        every lane rewrites its column from the one stage into the other -- token by token, each number from its
//                        known end backwards -- and the round's bytes leave by line_store.  A round ends with the last sample whose
//                        column ends inside the input stage and whose text ends inside the output stage.  With a sample map the
//                        lanes read their columns in place from global memory (as vcfdec_parse_kernel does) and only the output
//                        is staged.  A column longer than the input stage is read from global memory by its lane, a text longer
//                        than the output stage written there byte by byte by its lane: one sample a round then, at the offset the
//                        scan of the rounds before gave it, so no byte falls outside the site's [d_off[k], d_off[k + 1]).
#include <hipcub/hipcub.hpp>
#include <vector>
#include "bcfcodec.h"

using namespace bcfgpu;

static_assert(sizeof(bcfgpu_vcf_rewrite) == 32, "bcfgpu_vcf_rewrite is 32 bytes");

namespace bcfgpu {

constexpr int RW_STAGE = COD_SLICE;                             // payload bytes of either stage
constexpr uint32_t RW_MAX_RUN = 1u << 30;                       // the longest run: lengths and offsets inside a site's work are int
static_assert(RW_STAGE % COD_LINE == 0, "the stages are whole lines");
static_assert(BCFGPU_VCF_REWRITE_MAX_KEYS <= 64, "r_mask has a bit a key");

struct CallRwArgs {
    const bcfgpu_call_site *site;
    const int8_t *gt;
    const int32_t *pl, *gq;
    int n_gt_max;
    const unsigned char *text;
    const bcfgpu_vcf_vec *vec;          // [n_sites]: off and len as the indexing kernel reads them
    const bcfgpu_vcf_rewrite *rec;      // [n_sites]
    const int32_t *col;                 // [n_smpl] or nullptr
    int n_smpl_in, n_smpl;
};

// what is the same for every sample of a site
struct RwSite {
    unsigned long long r_mask;
    int n_fmt, pl_idx, nals, nn, ngn, flags;
    uint32_t inv;                       // four bits an output place t < 5: the input value that goes there, 15: none ('.')
};

__device__ __forceinline__ RwSite rw_site(const CallRwArgs &A, int k)
{
    const bcfgpu_vcf_rewrite r = A.rec[k];
    const bcfgpu_call_site c = A.site[k];
    RwSite R;
    R.r_mask = r.r_mask; R.n_fmt = r.n_fmt; R.pl_idx = r.pl_idx; R.nals = r.nals; R.flags = r.flags;
    R.nn = c.nals_new < 1 ? 1 : c.nals_new > BCFGPU_MAX_ALLELES ? BCFGPU_MAX_ALLELES : c.nals_new;
    R.ngn = R.nn * (R.nn + 1) / 2; if (R.ngn > A.n_gt_max) R.ngn = A.n_gt_max;
    R.inv = 0xfffffu;
    #pragma unroll
    for (int i = 0; i < BCFGPU_MAX_ALLELES; ++i) {              // out[map[i]] = value[i] in turn: the last one stays
        const int t = c.als_map[i];
        if (i < R.nals && t >= 0 && t < BCFGPU_MAX_ALLELES) R.inv = (R.inv & ~(15u << (4 * t))) | ((uint32_t)i << (4 * t));
    }
    return R;
}

// bytes p[a, b) to o
template <bool WRITE>
__device__ __forceinline__ int copy_bytes(unsigned char *o, const unsigned char *p, int a, int b)
{
    if (WRITE) for (int j = a; j < b; ++j) o[j - a] = p[j];
    return b - a;
}

// The text of called sample s at site k: its input column is p[0, n), p[0] the tab in front of it (LDS or global memory).  Its
// length, and with WRITE its bytes at o (LDS or global memory).
template <bool WRITE>
__device__ __forceinline__ int rw_sample(const CallRwArgs &A, const RwSite &R, size_t k, int s, const unsigned char *p, int n, unsigned char *o)
{
    const size_t S = (size_t)A.n_smpl;
    int len = 1;
    if (WRITE) o[0] = '\t';
    {
        const int g0 = A.gt[(k * 2 + 0) * S + s], g1 = A.gt[(k * 2 + 1) * S + s];
        if (WRITE) o[len] = gt_char(g0);
        ++len;
        if (g1 != BCFGPU_GT_VECTOR_END) {
            if (WRITE) { o[len] = '/'; o[len + 1] = gt_char(g1); }
            len += 2;
        }
    }
    int i = 1;                                                  // where the next token starts
    bool more = true;                                           // the column has a token there (an empty one too); else: '.'
    for (int f = 0; f < R.n_fmt; ++f) {
        int e = i;
        if (more) while (e < n && p[e] != ':') ++e;             // the token is p[i, e)
        if (f == R.pl_idx) {
            if (R.flags & 1) {
                if (WRITE) o[len] = ':';
                ++len;
                const int32_t *q = A.pl + k * A.n_gt_max * S + s;
                int j = 0;
                for (; j < R.ngn; ++j) {
                    const int32_t v = q[(size_t)j * S];
                    if (v == BCFGPU_INT32_VECTOR_END) break;
                    if (j) { if (WRITE) o[len] = ','; ++len; }
                    len += text_value<WRITE>(o + len, v);
                }
                if (j == 0) { if (WRITE) o[len] = '.'; ++len; }
            }
        } else {
            if (WRITE) o[len] = ':';
            ++len;
            bool remap = more && (R.r_mask >> f & 1ull) && R.nn != R.nals;
            if (remap) {                                        // only a token of one value an allele follows the alleles
                int nv = 1;
                for (int j = i; j < e; ++j) nv += p[j] == ',';
                remap = nv == R.nals;
            }
            if (!more) { if (WRITE) o[len] = '.'; ++len; }
            else if (!remap) len += copy_bytes<WRITE>(o + len, p, i, e);
            else for (int t = 0; t < R.nn; ++t) {
                const int src = R.nn == 1 ? 0 : (int)(R.inv >> (4 * t) & 15u);
                if (t) { if (WRITE) o[len] = ','; ++len; }
                if (src == 15) { if (WRITE) o[len] = '.'; ++len; continue; }
                int a = i;
                for (int c = 0; c < src; ++a) c += p[a] == ',';         // (the token has nals values: src commas lie inside it)
                int b = a;
                while (b < e && p[b] != ',') ++b;
                len += copy_bytes<WRITE>(o + len, p, a, b);
            }
        }
        if (more) { if (e < n) i = e + 1; else more = false; }
    }
    if (R.flags & 2) {
        if (WRITE) o[len] = ':';
        ++len;
        len += text_value<WRITE>(o + len, A.gq[k * S + s]);
    }
    return len;
}

// size[k0 + b] = bytes of the site's text (0: no record); the last workgroup of the last chunk sets size[n_sites] = 0
__global__ __launch_bounds__(COD_THREADS) void callrw_size_kernel(CallRwArgs A, const uint8_t *emit, int k0, int nk, int n_sites, const uint32_t *start,
                                                                  unsigned long long *size)
{
    __shared__ unsigned long long red[COD_THREADS / 64];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= nk) { if (tid == 0) size[n_sites] = 0; return; }
    const int k = k0 + blockIdx.x;
    if (emit && !emit[k]) { if (tid == 0) size[k] = 0; return; }
    const RwSite R = rw_site(A, k);
    const unsigned char *run = A.text + A.vec[k].off;
    const uint32_t *st = start + (size_t)blockIdx.x * ((size_t)A.n_smpl_in + 1);
    unsigned long long b = 0;
    for (int s = tid; s < A.n_smpl; s += COD_THREADS) {
        const int c = A.col ? A.col[s] : s;
        b += (unsigned long long)rw_sample<false>(A, R, (size_t)k, s, run + st[c], (int)(st[c + 1] - st[c]), nullptr);
    }
    for (int d = 32; d; d >>= 1) b += __shfl_xor(b, d, 64);
    if ((tid & 63) == 0) red[tid >> 6] = b;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < COD_THREADS / 64; ++w) t += red[w];
        size[k] = t;
    }
}

// how many lanes of the workgroup hold `pred`: a ballot a wavefront, the counts through cnt[COD_THREADS / 64] (LDS).  Every lane of the
// workgroup calls it; cnt is free again when it returns
__device__ __forceinline__ int wg_count(bool pred, int *cnt, int tid)
{
    const unsigned long long m = __ballot(pred);
    if ((tid & 63) == 0) cnt[tid >> 6] = __popcll(m);
    __syncthreads();
    int c = 0;
    #pragma unroll
    for (int w = 0; w < COD_THREADS / 64; ++w) c += cnt[w];
    __syncthreads();
    return c;
}

__global__ __launch_bounds__(COD_THREADS) void callrw_write_kernel(CallRwArgs A, int k0, const uint32_t *start, const unsigned long long *off, unsigned char *buf)
{
    typedef hipcub::BlockScan<int, COD_THREADS> Scan;
    __shared__ __attribute__((aligned(16))) unsigned char in_stage[COD_LINE + RW_STAGE];
    __shared__ __attribute__((aligned(16))) unsigned char out_stage[COD_LINE + RW_STAGE];
    // the scan's storage, the wavefronts' counts and the word that hands the round's size to every lane lie in the output stage: a
    // round is through with them before its first byte goes there, so the workgroup takes the two stages of bcfkeys.hip and not a
    // byte more
    constexpr int N_WORDS = COD_THREADS / 64 + 1;
    static_assert(sizeof(typename Scan::TempStorage) % 4 == 0 && sizeof(typename Scan::TempStorage) + 4 * N_WORDS <= sizeof out_stage, "scan storage inside the stage");
    typename Scan::TempStorage &scan_tmp = *reinterpret_cast<typename Scan::TempStorage*>(out_stage);
    int *cnt = reinterpret_cast<int*>(out_stage + sizeof(typename Scan::TempStorage));
    int &round_bytes = cnt[COD_THREADS / 64];
    const int k = k0 + blockIdx.x, tid = threadIdx.x;
    if (off[k + 1] == off[k]) return;                                       // no record at this site
    const RwSite R = rw_site(A, k);
    const unsigned char *run = A.text + A.vec[k].off;
    const uint32_t *st = start + (size_t)blockIdx.x * ((size_t)A.n_smpl_in + 1);
    const int n_smpl = A.n_smpl;
    unsigned char *g = buf + off[k];                                        // where the round's first byte goes
    for (int s0 = 0; s0 < n_smpl; ) {
        const int s = s0 + tid;
        // the input side: the lanes that have their column at hand this round are the first `lanes`, and p[0, n) is the column
        const unsigned char *p = run;
        int n = 0, lanes;
        if (A.col) {                                                        // a sample map: every lane its own column, in place
            lanes = n_smpl - s0 < COD_THREADS ? n_smpl - s0 : COD_THREADS;
            if (tid < lanes) { const int c = A.col[s]; p = run + st[c]; n = (int)(st[c + 1] - st[c]); }
        } else {
            // the samples from s0 on whose columns end inside the stage (the first `lanes` ones: the ends only grow)
            const uint32_t b0 = st[s0], b = s < n_smpl ? st[s] : 0u, e = s < n_smpl ? st[s + 1] : 0u;
            lanes = wg_count(s < n_smpl && e - b0 <= (uint32_t)RW_STAGE, cnt, tid);
            n = (int)(e - b);
            if (lanes == 0) { lanes = 1; p = run + b; }                     // one column longer than the stage: lane 0 reads it where it lies
            else {
                const int sh = line_load(in_stage, run + b0, (int)(st[s0 + lanes] - b0), tid);
                __syncthreads();
                p = in_stage + sh + (b - b0);
            }
        }
        // the output side: the lengths and where each text starts in the round; the round ends with the last sample whose text ends
        // inside the stage (a length past the stage counts as the stage and a byte: the scan's sums stay small)
        const int len = tid < lanes ? rw_sample<false>(A, R, (size_t)k, s, p, n, nullptr) : 0;
        const int clen = len > RW_STAGE ? RW_STAGE + 1 : len;
        int at;
        Scan(scan_tmp).ExclusiveSum(clen, at);
        const bool in = tid < lanes && at + clen <= RW_STAGE;
        const int fit = wg_count(in, cnt, tid);
        if (tid == (fit ? fit - 1 : 0)) round_bytes = fit ? at + len : len;
        __syncthreads();
        const int nb = round_bytes;
        __syncthreads();                                                    // (the stage is free for the texts from here)
        if (fit == 0) {                                                     // one text longer than the stage: lane 0 writes it where it goes
            if (tid == 0) rw_sample<true>(A, R, (size_t)k, s, p, n, g);
        } else {
            const int sh = line_shift(g);
            // Lanes read and write single bytes at offsets that depend on the columns before them: how these meet on the banks is not measured
            if (in) rw_sample<true>(A, R, (size_t)k, s, p, n, out_stage + sh + at);
            __syncthreads();
            line_store(out_stage, g, nb, tid);
        }
        __syncthreads();
        g += nb; s0 += fit ? fit : 1;
    }
}

}  // namespace bcfgpu

extern "C" int bcfgpu_call_rewrite_vcf(bcfgpu_ctx *ctx, int32_t n_sites, int32_t n_gt_max, const bcfgpu_call_out *planes,
                                       const bcfgpu_vcf_rewrite *rec, int32_t n_smpl_in,
                                       const void *d_text, uint64_t n_text_bytes, const int32_t *col,
                                       const uint8_t *d_emit, void *d_buf, uint64_t cap_bytes, uint64_t *d_off, uint64_t *n_bytes)
{
    if (!n_bytes) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_rewrite_vcf: bad arguments");
    *n_bytes = 0;
    if (!ctx || !planes || !d_off || n_sites < 0 || n_smpl_in < 1 || n_gt_max < 1 || n_gt_max > BCFGPU_MAX_PL || (cap_bytes && !d_buf) ||
        (n_text_bytes && !d_text) || (n_sites && (!rec || !planes->site || !planes->gt)))
        return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_rewrite_vcf: bad arguments");
    if ((uint64_t)n_sites + 1 > (uint64_t)INT32_MAX) return bcfgpu_set_error(BCFGPU_E_RANGE, "bcfgpu_call_rewrite_vcf: too many sites for one call");
    hipStream_t st;
    if (bcfgpu_internal_device(ctx, &st, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_rewrite_vcf: bad context");
    const int S = bcfgpu_internal_cfg(ctx)->n_smpl;
    if (S < 1 || (!col && S > n_smpl_in)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_rewrite_vcf: more called samples than input samples and no sample map");
    if (col) for (int s = 0; s < S; ++s) if (col[s] < 0 || col[s] >= n_smpl_in) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_rewrite_vcf: a sample map entry outside the input samples");
    std::vector<bcfgpu_vcf_vec> vec((size_t)n_sites);
    for (int k = 0; k < n_sites; ++k) {
        const bcfgpu_vcf_rewrite &r = rec[k];
        if (r.n_fmt < 1 || r.n_fmt > BCFGPU_VCF_REWRITE_MAX_KEYS) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_rewrite_vcf: a record has no or more than 64 FORMAT keys");
        if (r.nals < 1 || r.nals > BCFGPU_MAX_ALLELES) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_rewrite_vcf: a record has no or more than 5 alleles");
        if (r.pl_idx >= r.n_fmt) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_rewrite_vcf: PL's place is outside the record's FORMAT keys");
        if ((r.flags & 1) && (r.pl_idx < 0 || !planes->pl)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_rewrite_vcf: PL is listed and the record has no PL or the plane is NULL");
        if ((r.flags & 2) && !planes->gq) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_rewrite_vcf: GQ is listed and its plane is NULL");
        vec[k].off = r.off; vec[k].len = r.len; vec[k].idx = r.pl_idx;
    }
    for (int k = 0; k < n_sites; ++k) {
        if (rec[k].len > n_text_bytes || rec[k].off > n_text_bytes - rec[k].len) return bcfgpu_set_error(BCFGPU_E_RANGE, "bcfgpu_call_rewrite_vcf: a record's columns run past the end of the text");
        if (rec[k].len > RW_MAX_RUN) return bcfgpu_set_error(BCFGPU_E_RANGE, "bcfgpu_call_rewrite_vcf: a record's columns are longer than 1 GiB");
    }
    if (n_sites == 0) return enc_offsets(ctx, st, "bcfgpu_call_rewrite_vcf", d_off, 1, cap_bytes, n_bytes);
    // the offsets of one site's columns, and how many sites' offsets the slot takes at once (as bcfgpu_call_decode_vcf)
    const size_t per = (size_t)n_smpl_in + 1, fits = BCFGPU_VCFDEC_START_BYTES / 4 / per;
    const int chunk = fits < 1 ? 1 : fits < (size_t)n_sites ? (int)fits : n_sites;
    const bool once = chunk == n_sites;
    CallRwArgs A;
    A.site = planes->site; A.gt = planes->gt; A.pl = planes->pl; A.gq = planes->gq; A.n_gt_max = n_gt_max;
    A.text = (const unsigned char*)d_text; A.n_smpl_in = n_smpl_in; A.n_smpl = S;
    A.vec = (const bcfgpu_vcf_vec*)ws_upload(ctx, WS_COMPACT_VCFRW_VEC, vec.data(), vec.size() * sizeof vec[0], 64, st);
    A.rec = (const bcfgpu_vcf_rewrite*)ws_upload(ctx, WS_COMPACT_VCFRW_REC, rec, (size_t)n_sites * sizeof *rec, 64, st);
    A.col = col ? (const int32_t*)ws_upload(ctx, WS_COMPACT_VCFRW_COL, col, (size_t)S * 4, 64, st) : nullptr;
    uint32_t *d_start = (uint32_t*)bcfgpu_internal_ws(ctx, WS_COMPACT_VCFRW_START, (size_t)chunk * per * 4);
    uint32_t *d_err = (uint32_t*)bcfgpu_internal_ws(ctx, WS_COMPACT_VCFRW_ERR, 4);
    uint32_t *h_err = (uint32_t*)bcfgpu_internal_pinned(ctx, PIN_VCFRW_ERR, 4);
    if (!A.vec || !A.rec || (col && !A.col) || !d_start || !d_err || !h_err) { (void)hipStreamSynchronize(st); return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_call_rewrite_vcf: workspace"); }
    // the indexing pass over every site before anything is written: with the offsets when they all fit the slot, else counting only
    // (`vec` is read by its copy until the stream is through)
    if (hipMemsetAsync(d_err, 0xff, 4, st) != hipSuccess) { (void)hipStreamSynchronize(st); return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_rewrite_vcf: error word"); }
    launch_vcfdec_index(A.text, A.vec, 0, n_sites, n_smpl_in, once ? d_start : nullptr, d_err, st);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h_err, d_err, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_rewrite_vcf: indexing pass");
    if (h_err[0] != VDEC_NO_ERROR) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_rewrite_vcf: a record does not hold n_smpl_in sample columns, each behind a tab");
    unsigned long long *off = reinterpret_cast<unsigned long long*>(d_off);
    for (int k0 = 0; k0 < n_sites; k0 += chunk) {
        const int nk = n_sites - k0 < chunk ? n_sites - k0 : chunk, last = k0 + nk == n_sites;
        if (!once) launch_vcfdec_index(A.text, A.vec, k0, nk, n_smpl_in, d_start, d_err, st);
        hipLaunchKernelGGL(callrw_size_kernel, dim3(nk + last), dim3(COD_THREADS), 0, st, A, d_emit, k0, nk, n_sites, d_start, off);
    }
    const int rc = enc_offsets(ctx, st, "bcfgpu_call_rewrite_vcf", d_off, n_sites + 1, cap_bytes, n_bytes);
    if (rc || *n_bytes == 0) { (void)hipStreamSynchronize(st); return rc; }
    for (int k0 = 0; k0 < n_sites; k0 += chunk) {
        const int nk = n_sites - k0 < chunk ? n_sites - k0 : chunk;
        if (!once) launch_vcfdec_index(A.text, A.vec, k0, nk, n_smpl_in, d_start, d_err, st);
        hipLaunchKernelGGL(callrw_write_kernel, dim3(nk), dim3(COD_THREADS), 0, st, A, k0, d_start, off, (unsigned char*)d_buf);
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_rewrite_vcf: write pass");
    return 0;
}
