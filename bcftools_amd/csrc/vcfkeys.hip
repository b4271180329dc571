// vcfkeys.hip -- the pass-through integer FORMAT keys of a call record (AD, ADF, ADR, DP, SP, ...) as BCF2 key blocks, made on the
// device from the input record's own text: what the text route does per written record of VCF text input on one host thread -- the
// columns split at tabs, every column at ':', every Number=R token at ',' and printed again in the alleles' new order
// (print_sample_text / print_numberR of host/bcfgpu_call.c), then split and parsed a second time and narrowed to the smallest integer
// type (split_samples / encode_fmt_key / int_val / enc_vint of host/vcfio.c).  bcfkeys.hip with the input as text: vcfdec.hip's
// reading end joined to bcfkeys.hip's writing end:
//   a called sample reads input column col[s] (or s); the column is cut at ':', token idx is the key's text ('.' when the column has
//   fewer tokens), cut at ',' into its values: '.' is `missing`, anything else [+-]?[0-9]+ inside int32;
//   Number=R and alleles dropped (nals_new != nals) and the token present with one value per allele: [v[0]] when one allele is left,
//   else nals_new values `missing` with out[als_map[i]] = v[i] for the kept alleles; in every other case the values as they are;
//   the record's width is the longest vector over the called samples (shorter ones padded with `end of vector`), its type the
//   smallest of int8 / int16 / int32 that holds every output value which is no sentinel (-120 .. 127, -32760 .. 32767).
// A job one of whose values the exact grammar refuses (an empty value, `12x`, a blank, a number past int32: strtol would make
// something of each) or whose width passes BCFGPU_BCF_KEY_MAX_WIDTH is flagged in status[] and has no block: its caller makes it.
//
//   vcfdec_index_kernel  (vcfdec.hip, launch_vcfdec_index) the offsets of every column's tab inside its record's run, and the check
//                        that the run is n_smpl_in columns: over the sites that have a job with a record
//   keytxt_size_kernel   one workgroup a key job, a lane a called sample: the column walked where it lies in global memory to token
//                        idx, its values parsed; the output vector's length, largest value, largest negated value and the status
//                        bits (wavefront shuffles, then LDS) -> the block's width, type and size, one packed word a job
//   enc_offsets          the blocks' offsets (the device scan, gather.hip)
//   keytxt_write_kernel  one workgroup a key job: the header bytes, then the values in rounds of called samples.  Without a sample map
//                        the columns of a round's samples are one span of the run: it comes into the input stage by line_load, a lane
//                        a called sample parses its token there and puts its values into the output stage at their place in the
//                        record; from there 16 bytes a lane to consecutive addresses (line_store).  A round ends with the last sample
//                        whose column ends inside the input stage and whose values end inside the output stage.  A column longer
//                        than the stage is read from global memory by its lane; with a sample map every lane reads its column
//                        from global memory (as vcfdec_parse_kernel does) and only the output is staged.
// A workgroup a job, not a workgroup a site: a record's jobs walk its columns once each (see DESIGN.md 3.6 for why this form stands).
// Numbers are parsed forward, a byte at a time; the at most five values of a remapped token live in registers and find their places
// by unrolled selects: no array is indexed with a run-time value, no kernel has a private segment.
#include <vector>
#include "bcfcodec.h"

using namespace bcfgpu;

static_assert(sizeof(bcfgpu_vcf_key) == 32, "bcfgpu_vcf_key is 32 bytes");

namespace bcfgpu {

constexpr int KTXT_NRED = 4;                                    // width, max, -min, status
constexpr int KTXT_STAGE = COD_SLICE;                           // payload bytes of either stage
constexpr uint32_t KTXT_MAX_RUN = 1u << 30;                     // the longest run: offsets inside a site's work are int

static_assert(BCFGPU_BCF_KEY_MAX_WIDTH * 4 <= KTXT_STAGE, "a sample of the widest key fits the output stage: a round is at least 15 samples");
static_assert(BCFGPU_MAX_ALLELES == 5, "the remapped token's values are five registers, four bits a place in inv");

// what is the same for every sample of a job.  On the device a job's reserved[0] is its run's place among the indexed runs (-1: its
// site has no record): the entry fills it in its uploaded copy
struct KtJob {
    int idx, nals, nn;
    bool remap;                         // Number=R and alleles dropped: a token with nals values follows the alleles
    uint32_t inv;                       // four bits an output place t < 5: the input value that goes there, 15: none (`missing`)
};

__device__ __forceinline__ KtJob ktxt_job(const bcfgpu_vcf_key &J, const bcfgpu_call_site &c)
{
    KtJob K;
    K.idx = J.idx; K.nals = J.nals;
    K.nn = c.nals_new < 1 ? 1 : c.nals_new > BCFGPU_MAX_ALLELES ? BCFGPU_MAX_ALLELES : c.nals_new;
    K.remap = (J.flags & 1) && K.nn != K.nals;
    K.inv = 0xfffffu;
    #pragma unroll
    for (int i = 0; i < BCFGPU_MAX_ALLELES; ++i) {              // out[map[i]] = value[i] in turn: the last one stays
        const int t = c.als_map[i];
        if (i < K.nals && t >= 0 && t < BCFGPU_MAX_ALLELES) K.inv = (K.inv & ~(15u << (4 * t))) | ((uint32_t)i << (4 * t));
    }
    if (K.nn == 1) K.inv = 0xffff0u;                            // [v[0]]
    return K;
}

// the column p[0, n), p[0] its tab: i = the first byte of token idx; false: the column has fewer tokens (the token is '.')
__device__ __forceinline__ bool ktxt_token(const unsigned char *p, int n, int idx, int &i)
{
    int f = 0;
    for (i = 1; f < idx && i < n; ++i) f += p[i] == ':';
    return f == idx;
}

// value `src` of the five (15, or a place past them: `missing`)
__device__ __forceinline__ int32_t ktxt_pick(const int32_t (&v)[BCFGPU_MAX_ALLELES], int src)
{
    int32_t x = BCFGPU_INT32_MISSING;
    #pragma unroll
    for (int u = 0; u < BCFGPU_MAX_ALLELES; ++u) if (src == u) x = v[u];
    return x;
}

__device__ __forceinline__ void ktxt_stat(int32_t x, int32_t &mx, int32_t &ng)
{
    if (!is_sentinel(x)) { mx = x > mx ? x : mx; ng = -x > ng ? -x : ng; }
}

// one called sample's column: the output vector's length into m[0], its values into m[1], m[2]; m[3] = 1 when a value of the token is
// malformed (every value is looked at, kept by the remap or not)
__device__ __forceinline__ void ktxt_measure(const KtJob &K, const unsigned char *p, int n, int32_t (&m)[KTXT_NRED])
{
    int i, olen = 1;
    int32_t mx = COD_NONE, ng = COD_NONE;
    if (ktxt_token(p, n, K.idx, i)) {
        int32_t v[BCFGPU_MAX_ALLELES] = { BCFGPU_INT32_MISSING, BCFGPU_INT32_MISSING, BCFGPU_INT32_MISSING, BCFGPU_INT32_MISSING, BCFGPU_INT32_MISSING };
        int nv = 0;
        for (;;) {
            int32_t x;
            if (!get_text_value(p, i, n, x)) { m[3] = 1; return; }
            #pragma unroll
            for (int t = 0; t < BCFGPU_MAX_ALLELES; ++t) if (nv == t) v[t] = x;
            ktxt_stat(x, mx, ng);
            ++nv;
            if (i == n || p[i] != ',') break;
            ++i;
        }
        olen = nv;
        if (K.remap && nv == K.nals) {                          // a value on a dropped allele does not count
            olen = K.nn; mx = ng = COD_NONE;
            #pragma unroll
            for (int t = 0; t < BCFGPU_MAX_ALLELES; ++t) if (t < K.nn) ktxt_stat(ktxt_pick(v, (int)(K.inv >> (4 * t) & 15u)), mx, ng);
        }
    }
    m[0] = olen > m[0] ? olen : m[0]; m[1] = mx > m[1] ? mx : m[1]; m[2] = ng > m[2] ? ng : m[2];
}

// size[j0 + b] = bytes of the job's block (0: its site has no record, or the job is flagged), word = type | width << 2, status as
// include/bcfgpu.h says; the workgroup behind the last job sets size[n_keys] = 0
__global__ __launch_bounds__(COD_THREADS) void keytxt_size_kernel(const unsigned char *text, const bcfgpu_vcf_vec *runs, const bcfgpu_vcf_key *jobs, const int32_t *col,
                                                                   const bcfgpu_call_site *site, int j0, int nj, int n_keys, int u0, const uint32_t *start,
                                                                   int n_smpl_in, int n_smpl, unsigned long long *size, uint32_t *word, uint8_t *status)
{
    __shared__ int32_t red[COD_THREADS / 64][KTXT_NRED];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= nj) { if (tid == 0) size[n_keys] = 0; return; }
    const int j = j0 + blockIdx.x;
    const bcfgpu_vcf_key J = jobs[j];
    const int u = J.reserved[0];
    if (u < 0) { if (tid == 0) { size[j] = 0; word[j] = 0; status[j] = 0; } return; }
    const KtJob K = ktxt_job(J, site[J.site]);
    const unsigned char *run = text + runs[u].off;
    const uint32_t *st = start + (size_t)(u - u0) * ((size_t)n_smpl_in + 1);
    int32_t m[KTXT_NRED] = { 1, COD_NONE, COD_NONE, 0 };
    for (int s = tid; s < n_smpl; s += COD_THREADS) {
        const int c = col ? col[s] : s;
        ktxt_measure(K, run + st[c], (int)(st[c + 1] - st[c]), m);
    }
    wg_max(m, red, tid);
    if (tid == 0) {
        const int w = m[0], t = int_type(m[1], m[2]);
        const int bad = m[3] ? 1 : w > BCFGPU_BCF_KEY_MAX_WIDTH ? 2 : 0;
        size[j] = bad ? 0ull : (unsigned long long)(id_bytes(J.key_id) + desc_bytes(w)) + (unsigned long long)n_smpl * (unsigned)w * (unsigned)elem_bytes(t);
        word[j] = bad ? 0u : (uint32_t)t | (uint32_t)w << 2;
        status[j] = (uint8_t)bad;
    }
}

// one called sample's w output values, as integers of `es` bytes, into q[0 .. w * es) (any alignment when bytewise).  The job is not
// flagged: every value of the token parses
template <bool BYTEWISE>
__device__ __forceinline__ void ktxt_put_sample(const KtJob &K, const unsigned char *p, int n, int w, int es, unsigned char *q)
{
    int i, j = 0;
    if (!ktxt_token(p, n, K.idx, i)) { put_int<BYTEWISE>(q, narrow(BCFGPU_INT32_MISSING, es), es); j = 1; }
    else {
        bool remap = K.remap;
        if (remap) {                                            // only a token of one value an allele follows the alleles
            int nv = 1;
            for (int a = i; a < n && p[a] != ':'; ++a) nv += p[a] == ',';
            remap = nv == K.nals;
        }
        if (remap) {
            int32_t v[BCFGPU_MAX_ALLELES] = { BCFGPU_INT32_MISSING, BCFGPU_INT32_MISSING, BCFGPU_INT32_MISSING, BCFGPU_INT32_MISSING, BCFGPU_INT32_MISSING };
            #pragma unroll
            for (int t = 0; t < BCFGPU_MAX_ALLELES; ++t) {
                if (t >= K.nals) continue;
                int32_t x;
                get_text_value(p, i, n, x);
                v[t] = x;
                ++i;                                            // (the ',' behind it; behind the last value i is not read again)
            }
            #pragma unroll
            for (int t = 0; t < BCFGPU_MAX_ALLELES; ++t)
                if (t < K.nn && t < w) put_int<BYTEWISE>(q + t * es, narrow(ktxt_pick(v, (int)(K.inv >> (4 * t) & 15u)), es), es);
            j = K.nn < w ? K.nn : w;
        } else for (; j < w; ) {                                // (no more than w values: the size pass saw the same text)
            int32_t x;
            get_text_value(p, i, n, x);
            put_int<BYTEWISE>(q + j * es, narrow(x, es), es);
            ++j;
            if (i >= n || p[i] != ',') break;
            ++i;
        }
    }
    for (; j < w; ++j) put_int<BYTEWISE>(q + j * es, narrow(BCFGPU_INT32_VECTOR_END, es), es);
}

__global__ __launch_bounds__(COD_THREADS) void keytxt_write_kernel(const unsigned char *text, const bcfgpu_vcf_vec *runs, const bcfgpu_vcf_key *jobs, const int32_t *col,
                                                                    const bcfgpu_call_site *site, int j0, int u0, const uint32_t *start, int n_smpl_in, int n_smpl,
                                                                    const unsigned long long *off, const uint32_t *word, unsigned char *buf)
{
    __shared__ __attribute__((aligned(16))) unsigned char in_stage[COD_LINE + KTXT_STAGE], out_stage[COD_LINE + KTXT_STAGE];
    const int j = j0 + blockIdx.x, tid = threadIdx.x;
    if (off[j + 1] == off[j]) return;                                       // no record at this job's site, or a flagged job
    const bcfgpu_vcf_key J = jobs[j];
    const int u = J.reserved[0];
    if (u < 0) return;
    const KtJob K = ktxt_job(J, site[J.site]);
    const unsigned char *run = text + runs[u].off;
    const uint32_t *st = start + (size_t)(u - u0) * ((size_t)n_smpl_in + 1);
    const uint32_t wd = word[j];
    const int t = (int)(wd & 3u), es = elem_bytes(t), w = (int)(wd >> 2), id = J.key_id;
    unsigned char *dst = buf + off[j];
    if (tid == 0) put_header(dst, id, w, t);
    dst += id_bytes(id) + desc_bytes(w);
    const int per_o = w * es;                                               // bytes a sample in the record (w >= 1)
    const int slice_o = KTXT_STAGE / per_o < COD_THREADS ? KTXT_STAGE / per_o : COD_THREADS;      // samples a round on the output side
    for (int s0 = 0; s0 < n_smpl; ) {
        const int s = s0 + tid;
        // the input side: the first `cs` lanes have their column at hand this round, p[0, n)
        const unsigned char *p = run;
        int n = 0, cs;
        if (col) {                                                          // a sample map: every lane its own column, in place
            cs = n_smpl - s0 < slice_o ? n_smpl - s0 : slice_o;
            if (tid < cs) { const int c = col[s]; p = run + st[c]; n = (int)(st[c + 1] - st[c]); }
        } else {
            // the samples from s0 on whose columns end inside the input stage and whose values end inside the output stage (the
            // first `cs` ones: the ends only grow)
            const uint32_t b0 = st[s0], b = s < n_smpl ? st[s] : 0u, e = s < n_smpl ? st[s + 1] : 0u;
            cs = __syncthreads_count(s < n_smpl && tid < slice_o && e - b0 <= (uint32_t)KTXT_STAGE);
            n = (int)(e - b);
            if (cs == 0) { cs = 1; p = run + b; }                           // one column longer than the stage: lane 0 reads it where it lies
            else {
                const int sh = line_load(in_stage, run + b0, (int)(st[s0 + cs] - b0), tid);
                __syncthreads();
                p = in_stage + sh + (b - b0);
            }
        }
        unsigned char *g = dst + (size_t)s0 * per_o;                        // where the round's first byte goes
        const int sh = line_shift(g), nb = cs * per_o;
        unsigned char *q = out_stage + sh + (size_t)tid * per_o;
        const bool bytewise = sh % es != 0;                                 // values that straddle their natural alignment: byte by byte
        // Lanes read single bytes at offsets that depend on the columns before them and write `per_o` bytes apart (the pattern of
        // bcfkeys.hip's output side): how these meet on the banks is not measured
        if (tid < cs) { if (bytewise) ktxt_put_sample<true>(K, p, n, w, es, q); else ktxt_put_sample<false>(K, p, n, w, es, q); }
        __syncthreads();
        line_store(out_stage, g, nb, tid);
        __syncthreads();
        s0 += cs;
    }
}

}  // namespace bcfgpu

extern "C" int bcfgpu_call_parse_keys_vcf(bcfgpu_ctx *ctx, int32_t n_keys, const bcfgpu_vcf_key *keys, int32_t n_sites, const bcfgpu_vcf_vec *run,
                                          int32_t n_smpl_in, const void *d_text, uint64_t n_text_bytes, const int32_t *col,
                                          const bcfgpu_call_site *d_site, const uint8_t *d_emit,
                                          void *d_buf, uint64_t cap_bytes, uint64_t *d_off, uint64_t *n_bytes, uint8_t *status)
{
    static const char *const name = "bcfgpu_call_parse_keys_vcf";
    if (!n_bytes) return bcfgpu_set_error(BCFGPU_E_ARG, name, "bad arguments");
    *n_bytes = 0;
    if (!ctx || !d_off || n_keys < 0 || n_sites < 0 || n_smpl_in < 1 || (cap_bytes && !d_buf) || (n_text_bytes && !d_text) ||
        (n_keys && (!keys || !d_site || !status)) || (n_sites && !run))
        return bcfgpu_set_error(BCFGPU_E_ARG, name, "bad arguments");
    if ((uint64_t)n_keys + 1 > (uint64_t)INT32_MAX) return bcfgpu_set_error(BCFGPU_E_RANGE, name, "too many keys for one call");
    hipStream_t st;
    if (bcfgpu_internal_device(ctx, &st, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, name, "bad context");
    const int S = bcfgpu_internal_cfg(ctx)->n_smpl;
    if (S < 1 || (!col && S > n_smpl_in)) return bcfgpu_set_error(BCFGPU_E_ARG, name, "more called samples than input samples and no sample map");
    if (col) for (int s = 0; s < S; ++s) if (col[s] < 0 || col[s] >= n_smpl_in) return bcfgpu_set_error(BCFGPU_E_ARG, name, "a sample map entry outside the input samples");
    for (int j = 0; j < n_keys; ++j) {
        const bcfgpu_vcf_key &k = keys[j];
        if (k.site < 0 || k.site >= n_sites || k.key_id < 0) return bcfgpu_set_error(BCFGPU_E_ARG, name, "a key's site is outside the sites or its id negative");
        if (j && k.site < keys[j - 1].site) return bcfgpu_set_error(BCFGPU_E_ARG, name, "the keys' sites decrease");
        if (k.idx < 0 || k.idx >= BCFGPU_VCF_REWRITE_MAX_KEYS) return bcfgpu_set_error(BCFGPU_E_ARG, name, "a key's place is outside the 64 FORMAT keys");
        if ((k.flags & 1) && (k.nals < 1 || k.nals > BCFGPU_MAX_ALLELES)) return bcfgpu_set_error(BCFGPU_E_ARG, name, "a Number=R key of a record with no or more than 5 alleles");
        if (k.reserved[0] || k.reserved[1] || k.reserved[2]) return bcfgpu_set_error(BCFGPU_E_ARG, name, "a key's reserved words are not 0");
    }
    for (int k = 0; k < n_sites; ++k) {
        if (run[k].len > n_text_bytes || run[k].off > n_text_bytes - run[k].len) return bcfgpu_set_error(BCFGPU_E_RANGE, name, "a record's columns run past the end of the text");
        if (run[k].len > KTXT_MAX_RUN) return bcfgpu_set_error(BCFGPU_E_RANGE, name, "a record's columns are longer than 1 GiB");
    }
    if (n_keys == 0) return enc_offsets(ctx, st, name, d_off, 1, cap_bytes, n_bytes);
    // which sites have a record (the device's mask comes down: n_sites bytes), and from them the runs to index: one a site that has a
    // job with a record.  The jobs go up with their run's place in reserved[0]
    std::vector<uint8_t> emit;
    if (d_emit) {
        emit.resize((size_t)n_sites);
        if (hipMemcpyAsync(emit.data(), d_emit, (size_t)n_sites, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return bcfgpu_set_error(BCFGPU_E_HIP, name, "the records' mask");
    }
    std::vector<bcfgpu_vcf_key> job(keys, keys + n_keys);
    std::vector<bcfgpu_vcf_vec> runs;
    std::vector<int> first;                                     // the first job of every indexed run, and n_keys behind the last
    for (int j = 0; j < n_keys; ++j) {
        const int k = job[j].site;
        if (d_emit && !emit[(size_t)k]) { job[j].reserved[0] = -1; continue; }
        if (runs.empty() || job[first.back()].site != k) { first.push_back(j); bcfgpu_vcf_vec v = run[k]; v.idx = 0; runs.push_back(v); }
        job[j].reserved[0] = (int32_t)runs.size() - 1;
    }
    const int n_runs = (int)runs.size();
    first.push_back(n_keys);
    if (n_runs) first[0] = 0;                                   // (the jobs without a record in front of the first run go with it)
    const int n_off = n_keys + 1;
    unsigned long long *off = reinterpret_cast<unsigned long long*>(d_off);
    // the offsets of one site's columns, and how many sites' offsets the slot takes at once (as bcfgpu_call_decode_vcf)
    const size_t per = (size_t)n_smpl_in + 1, fits = BCFGPU_VCFDEC_START_BYTES / 4 / per;
    const int chunk = fits < 1 ? 1 : fits < (size_t)n_runs ? (int)fits : n_runs;
    const bool once = chunk == n_runs;
    const bcfgpu_vcf_key *d_keys = (const bcfgpu_vcf_key*)ws_upload(ctx, WS_COMPACT_VCFKEY_JOBS, job.data(), job.size() * sizeof job[0], 64, st);
    const bcfgpu_vcf_vec *d_runs = n_runs ? (const bcfgpu_vcf_vec*)ws_upload(ctx, WS_COMPACT_VCFKEY_RUNS, runs.data(), runs.size() * sizeof runs[0], 64, st) : nullptr;
    const int32_t *d_col = col ? (const int32_t*)ws_upload(ctx, WS_COMPACT_VCFKEY_COL, col, (size_t)S * 4, 64, st) : nullptr;
    uint32_t *d_word = (uint32_t*)bcfgpu_internal_ws(ctx, WS_COMPACT_VCFKEY_WORD, (size_t)n_keys * 4 + 64);
    uint8_t *d_status = (uint8_t*)bcfgpu_internal_ws(ctx, WS_COMPACT_VCFKEY_STATUS, (size_t)n_keys + 64);
    uint32_t *d_start = (uint32_t*)bcfgpu_internal_ws(ctx, WS_COMPACT_VCFKEY_START, (size_t)(chunk ? chunk : 1) * per * 4);
    uint32_t *d_err = (uint32_t*)bcfgpu_internal_ws(ctx, WS_COMPACT_VCFKEY_ERR, 4);
    uint32_t *h_err = (uint32_t*)bcfgpu_internal_pinned(ctx, PIN_VCFKEY_ERR, 4);
    if (!d_keys || (n_runs && !d_runs) || (col && !d_col) || !d_word || !d_status || !d_start || !d_err || !h_err) {
        (void)hipStreamSynchronize(st);
        return bcfgpu_set_error(BCFGPU_E_NOMEM, name, "workspace");
    }
    const unsigned char *text = (const unsigned char*)d_text;
    // the indexing pass over every run before anything is written: with the offsets when they all fit the slot, else counting only
    // (the host's vectors are read by their copies until the stream is through: every return below synchronises it)
    if (n_runs) {
        if (hipMemsetAsync(d_err, 0xff, 4, st) != hipSuccess) { (void)hipStreamSynchronize(st); return bcfgpu_set_error(BCFGPU_E_HIP, name, "error word"); }
        launch_vcfdec_index(text, d_runs, 0, n_runs, n_smpl_in, once ? d_start : nullptr, d_err, st);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h_err, d_err, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return bcfgpu_set_error(BCFGPU_E_HIP, name, "indexing pass");
        if (h_err[0] != VDEC_NO_ERROR) return bcfgpu_set_error(BCFGPU_E_ARG, name, "a record does not hold n_smpl_in sample columns, each behind a tab");
    }
    // the jobs of the runs [u0, u0 + nu) are [first[u0], first[u0 + nu)); without any run one launch sets every job's zeros
    for (int u0 = 0; u0 < n_runs || u0 == 0; u0 += chunk ? chunk : 1) {
        const int nu = n_runs - u0 < chunk ? n_runs - u0 : chunk, last = u0 + nu >= n_runs;
        const int j0 = n_runs ? first[u0] : 0, nj = (n_runs ? first[u0 + nu] : n_keys) - j0;
        if (!once && n_runs) launch_vcfdec_index(text, d_runs, u0, nu, n_smpl_in, d_start, d_err, st);
        hipLaunchKernelGGL(keytxt_size_kernel, dim3(nj + last), dim3(COD_THREADS), 0, st, text, d_runs, d_keys, d_col, d_site, j0, nj, n_keys, u0, d_start,
                           n_smpl_in, S, off, d_word, d_status);
    }
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(status, d_status, (size_t)n_keys, hipMemcpyDeviceToHost, st) != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return bcfgpu_set_error(BCFGPU_E_HIP, name, "size pass");
    }
    const int rc = enc_offsets(ctx, st, name, d_off, n_off, cap_bytes, n_bytes);
    if (rc || *n_bytes == 0) { (void)hipStreamSynchronize(st); return rc; }
    for (int u0 = 0; u0 < n_runs; u0 += chunk) {
        const int nu = n_runs - u0 < chunk ? n_runs - u0 : chunk;
        const int j0 = first[u0], nj = first[u0 + nu] - j0;
        if (!once) launch_vcfdec_index(text, d_runs, u0, nu, n_smpl_in, d_start, d_err, st);
        hipLaunchKernelGGL(keytxt_write_kernel, dim3(nj), dim3(COD_THREADS), 0, st, text, d_runs, d_keys, d_col, d_site, j0, u0, d_start, n_smpl_in, S, off, d_word,
                           (unsigned char*)d_buf);
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, name, "write pass");
    return 0;
}
