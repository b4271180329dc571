// bcfkeys.hip -- the pass-through integer FORMAT keys of a call record (AD, ADF, ADR, DP, SP, ...) as BCF2 key blocks, made on the
// device from the input record's bytes: what mcall_trim_and_update_numberR (mcall.c:1196-1265) does to the Number=R keys when
// alleles are dropped, bcf_subset to the samples, and the writer's typed-value encoder (bcf_enc_vint of htslib vcf.c; here
// host/vcfio.c enc_vint) to all of them, per record on one host thread.  The text route it stands for is vio_indiv_text, the
// record loop of host/bcfgpu_call.c with print_numberR, and encode_fmt_key / enc_vint of host/vcfio.c.  bcfdec.hip's reading end
// joined to bcfcallenc.hip's writing end:
//   a called sample reads input sample col[s] (or s); its vector v is its `width` values widened (int8 / int16 `missing` and `end
//   of vector` become the int32 sentinels) and cut at the first `end of vector`, an empty one being the one value `missing`;
//   Number=R and alleles dropped (nals_new != nals) and one value per allele: [v[0]] when one allele is left, else nals_new values
//   `missing` with out[als_map[i]] = v[i] for the kept alleles; in every other case v as it is;
//   the record's width is the longest vector over the called samples (shorter ones padded with `end of vector`), its type the
//   smallest of int8 / int16 / int32 that holds every output value which is no sentinel (-120 .. 127, -32760 .. 32767).
// Width and type are those of the output: both can be smaller than the input's.
//
//   keybcf_size_kernel   one workgroup a key job: the input run in slices of samples through the LDS stage of bcfdec.hip; per called
//                        sample the output vector's length, largest value and largest negated value (wavefront shuffles, then
//                        LDS) -> the block's width, type and size, one packed word a job
//   hipcub ExclusiveSum  the blocks' offsets
//   keybcf_write_kernel  one workgroup a key job: the header bytes, then the values in slices of called samples -- the input slice
//                        into one LDS stage (whole 16-byte lines, single bytes at both ends, from any byte alignment), a lane a
//                        called sample: its vector out of that stage, transformed, into a second stage at its place in the record;
//                        from there 16 bytes a lane to consecutive addresses (bcfcallenc.hip's store).
//                        With a sample map the called samples take their sample from the input stage: one load when the whole run
//                        fits a slice, else every input slice once per output slice.
// No straight copy of runs that come out as they went in: every block goes through the transform.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <cstdint>
#include "ctx.h"

using namespace bcfgpu;

static_assert(sizeof(bcfgpu_bcf_key) == 32, "bcfgpu_bcf_key is 32 bytes");

namespace bcfgpu {

constexpr int KENC_THREADS = 256;
constexpr int KENC_LINE = 16;                                   // bytes a lane loads / stores at once
constexpr int KENC_SLICE = BCFGPU_MAX_PL * 4 * 256;             // payload bytes of a slice in LDS (a sample is at most 255 x 4 bytes: >= 15 samples)
constexpr int KENC_NRED = 3;                                    // width, max, -min
constexpr int32_t KENC_NONE = INT32_MIN + 1;                    // "no value yet" of a maximum (enc_vint starts there)

static_assert(BCFGPU_BCF_KEY_MAX_WIDTH * 4 <= KENC_SLICE, "a sample of the widest key fits a slice");

__device__ __forceinline__ int kenc_id_bytes(int id) { return id <= 127 ? 2 : id <= 32767 ? 3 : 5; }     // a typed scalar: descriptor + value
__device__ __forceinline__ int kenc_desc_bytes(int w) { return w < 15 ? 1 : w <= 127 ? 3 : 4; }         // width >= 15: 0xF?, then the width as a typed int8 / int16
__device__ __forceinline__ int kenc_type(int32_t mx, int32_t neg_mn) { return mx <= 127 && neg_mn <= 120 ? 1 : mx <= 32767 && neg_mn <= 32760 ? 2 : 3; }
__device__ __forceinline__ bool kenc_sentinel(int32_t v) { return v == BCFGPU_INT32_MISSING || v == BCFGPU_INT32_VECTOR_END; }

// one input value, widened (dec_int: the smallest two values of int8 and int16 are `missing` and `end of vector`)
__device__ __forceinline__ int32_t kenc_value(const unsigned char *q, int es, bool aligned)
{
    if (es == 1) { const int32_t v = (int8_t)*q; return v == -128 ? BCFGPU_INT32_MISSING : v == -127 ? BCFGPU_INT32_VECTOR_END : v; }
    if (es == 2) {
        const int32_t v = aligned ? (int32_t)*reinterpret_cast<const int16_t*>(q) : (int32_t)(int16_t)(uint16_t)(q[0] | q[1] << 8);
        return v == -32768 ? BCFGPU_INT32_MISSING : v == -32767 ? BCFGPU_INT32_VECTOR_END : v;
    }
    if (aligned) return *reinterpret_cast<const int32_t*>(q);
    return (int32_t)((uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24);
}
// an output value as the integer of `es` bytes that stands for it: the sentinels are the type's own
__device__ __forceinline__ uint32_t kenc_narrow(int32_t v, int es)
{
    if (es == 4 || !kenc_sentinel(v)) return (uint32_t)v;
    return (es == 1 ? 0x80u : 0x8000u) | (uint32_t)(v == BCFGPU_INT32_VECTOR_END);
}

// what is the same for every sample of a job
struct KeyJob {
    const unsigned char *run;           // value [input sample 0][0]
    int es, width;                      // bytes a value and values a sample in the input (width 0: no values, every sample is '.')
    bool aligned;                       // the run's values lie at their natural alignment
    int nals, nn;                       // alleles of the input record, of the output record
    bool remap;                         // Number=R and alleles dropped: a sample with nals values follows the alleles
    int inv[BCFGPU_MAX_ALLELES];        // output value t is input value inv[t], -1: `missing`
};

__device__ __forceinline__ KeyJob kenc_job(const unsigned char *indiv, const bcfgpu_bcf_key &J, const bcfgpu_call_site &c)
{
    KeyJob K;
    K.run = indiv + J.off;
    K.es = J.type == 3 ? 4 : J.type == 0 ? 1 : J.type;
    K.width = J.type ? J.width : 0;
    K.aligned = ((uintptr_t)K.run & (uintptr_t)(K.es - 1)) == 0;
    K.nals = J.nals;
    K.nn = c.nals_new < 1 ? 1 : c.nals_new > BCFGPU_MAX_ALLELES ? BCFGPU_MAX_ALLELES : c.nals_new;
    K.remap = (J.flags & 1) && K.nn != K.nals;
    #pragma unroll
    for (int t = 0; t < BCFGPU_MAX_ALLELES; ++t) {
        K.inv[t] = -1;
        #pragma unroll
        for (int i = 0; i < BCFGPU_MAX_ALLELES; ++i) if (i < K.nals && c.als_map[i] == t) K.inv[t] = i;   // (the last one stays, as out[map[i]] = v[i] in turn leaves it)
    }
    if (K.nn == 1) K.inv[0] = 0;
    return K;
}

// the values of the sample at p before its first `end of vector`
__device__ __forceinline__ int kenc_len(const KeyJob &K, const unsigned char *p)
{
    int len = 0;
    for (; len < K.width; ++len) if (kenc_value(p + len * K.es, K.es, K.aligned) == BCFGPU_INT32_VECTOR_END) break;
    return len;
}

// the input run's bytes [0, nb) at g -> LDS at the offset g has inside a 16-byte line; returns that offset.  Whole lines in the middle,
// single bytes at both ends (bcfdec.hip's load).  The caller synchronises.
__device__ __forceinline__ int kenc_stage(unsigned char *stage, const unsigned char *g, int nb, int tid)
{
    const int sh = (int)((uintptr_t)g & (KENC_LINE - 1));
    const int lo = sh, hi = sh + nb;
    const int l0 = (lo + KENC_LINE - 1) / KENC_LINE, l1 = hi / KENC_LINE;   // whole lines [l0, l1)
    const unsigned char *ga = g - sh;
    if (l0 < l1) {
        for (int x = l0 + tid; x < l1; x += KENC_THREADS)
            reinterpret_cast<uint4*>(stage)[x] = reinterpret_cast<const uint4*>(ga)[x];
        const int head = l0 * KENC_LINE - lo, tail = hi - l1 * KENC_LINE;   // each < 16
        if (tid < head) stage[lo + tid] = ga[lo + tid];
        else if (tid >= 32 && tid - 32 < tail) stage[l1 * KENC_LINE + tid - 32] = ga[l1 * KENC_LINE + tid - 32];
    } else {
        for (int x = lo + tid; x < hi; x += KENC_THREADS) stage[x] = ga[x];  // fewer than 31 bytes, no whole line
    }
    return sh;
}

// one called sample (its input values at p; not read when the key has none): the output vector's length, its values into m[1], m[2]
__device__ __forceinline__ void kenc_measure(const KeyJob &K, const unsigned char *p, int32_t *m)
{
    const int len = kenc_len(K, p);
    int olen = len < 1 ? 1 : len;
    if (K.remap && olen == K.nals) {
        olen = K.nn;
        #pragma unroll
        for (int t = 0; t < BCFGPU_MAX_ALLELES; ++t) {
            if (t >= olen || K.inv[t] < 0 || len == 0) continue;
            const int32_t v = kenc_value(p + K.inv[t] * K.es, K.es, K.aligned);
            if (!kenc_sentinel(v)) { m[1] = v > m[1] ? v : m[1]; m[2] = -v > m[2] ? -v : m[2]; }
        }
    } else {
        for (int j = 0; j < len; ++j) {
            const int32_t v = kenc_value(p + j * K.es, K.es, K.aligned);
            if (!kenc_sentinel(v)) { m[1] = v > m[1] ? v : m[1]; m[2] = -v > m[2] ? -v : m[2]; }
        }
    }
    m[0] = olen > m[0] ? olen : m[0];
}

// size[j] = bytes of job j's block (0: its site has no record), size[n_keys] = 0; word[j] = type | width << 2
__global__ __launch_bounds__(KENC_THREADS) void keybcf_size_kernel(const unsigned char *indiv, const bcfgpu_bcf_key *jobs, const int32_t *col,
                                                                   const bcfgpu_call_site *site, const uint8_t *emit, int n_keys, int n_smpl_in, int n_smpl,
                                                                   unsigned long long *size, uint32_t *word)
{
    __shared__ __attribute__((aligned(16))) unsigned char stage[KENC_LINE + KENC_SLICE];
    __shared__ int32_t red[KENC_THREADS / 64][KENC_NRED];
    const int j = blockIdx.x, tid = threadIdx.x;
    if (j >= n_keys) { if (tid == 0) size[n_keys] = 0; return; }
    const bcfgpu_bcf_key J = jobs[j];
    if (emit && !emit[J.site]) { if (tid == 0) { size[j] = 0; word[j] = 0; } return; }
    const KeyJob K = kenc_job(indiv, J, site[J.site]);
    int32_t m[KENC_NRED] = { 1, KENC_NONE, KENC_NONE };
    const int per = K.width * K.es;                                         // bytes an input sample
    if (per) {
        const int slice = KENC_SLICE / per;                                 // input samples a slice
        for (int i0 = 0; i0 < n_smpl_in; i0 += slice) {
            if (!col && i0 >= n_smpl) break;                                // the input samples past the called ones
            const int ci = n_smpl_in - i0 < slice ? n_smpl_in - i0 : slice;
            const unsigned char *l = stage + kenc_stage(stage, K.run + (size_t)i0 * per, ci * per, tid);
            __syncthreads();
            if (col) {
                for (int s = tid; s < n_smpl; s += KENC_THREADS) {
                    const int c = col[s] - i0;
                    if (c >= 0 && c < ci) kenc_measure(K, l + (size_t)c * per, m);
                }
            } else {
                const int ce = i0 + ci < n_smpl ? ci : n_smpl - i0;
                for (int c = tid; c < ce; c += KENC_THREADS) kenc_measure(K, l + (size_t)c * per, m);
            }
            __syncthreads();
        }
    }                                                                       // no values: every sample is one `missing`, m as it starts
    #pragma unroll
    for (int i = 0; i < KENC_NRED; ++i)
        for (int d = 32; d; d >>= 1) { const int32_t o = __shfl_xor(m[i], d, 64); m[i] = o > m[i] ? o : m[i]; }
    if ((tid & 63) == 0) {
        #pragma unroll
        for (int i = 0; i < KENC_NRED; ++i) red[tid >> 6][i] = m[i];
    }
    __syncthreads();
    if (tid == 0) {
        #pragma unroll
        for (int i = 0; i < KENC_NRED; ++i)
            for (int w = 1; w < KENC_THREADS / 64; ++w) m[i] = red[w][i] > m[i] ? red[w][i] : m[i];
        int w = m[0];
        if (K.remap && per == 0 && K.nals == 1) w = K.nn;                   // ('.' is one value: at one allele it follows the alleles too)
        const int t = kenc_type(m[1], m[2]);
        size[j] = (unsigned long long)(kenc_id_bytes(J.key_id) + kenc_desc_bytes(w)) + (unsigned long long)n_smpl * (unsigned)w * (t == 3 ? 4u : (unsigned)t);
        word[j] = (uint32_t)t | (uint32_t)w << 2;
    }
}

// one called sample's w output values, as integers of `es` bytes, into q[0 .. w * es) (any alignment when bytewise)
template <bool BYTEWISE>
__device__ __forceinline__ void kenc_put_sample(const KeyJob &K, const unsigned char *p, int w, int es, unsigned char *q)
{
    const int len = K.width ? kenc_len(K, p) : 0;
    const bool remap = K.remap && (len < 1 ? 1 : len) == K.nals;
    const int olen = remap ? K.nn : len < 1 ? 1 : len;
    for (int j = 0; j < w; ++j) {
        int32_t x = BCFGPU_INT32_VECTOR_END;
        if (j < olen) {
            int src = j;                                                    // the input value that goes here, -1: `missing`
            if (remap) {
                src = -1;
                #pragma unroll
                for (int t = 0; t < BCFGPU_MAX_ALLELES; ++t) if (t == j) src = K.inv[t];
            }
            x = src < 0 || len == 0 ? BCFGPU_INT32_MISSING : kenc_value(p + src * K.es, K.es, K.aligned);
        }
        const uint32_t v = kenc_narrow(x, es);
        unsigned char *o = q + j * es;
        if (BYTEWISE) { for (int b = 0; b < es; ++b) o[b] = (unsigned char)(v >> (8 * b)); }
        else if (es == 1) *o = (unsigned char)v;
        else if (es == 2) *reinterpret_cast<uint16_t*>(o) = (uint16_t)v;
        else *reinterpret_cast<uint32_t*>(o) = v;
    }
}

__global__ __launch_bounds__(KENC_THREADS) void keybcf_write_kernel(const unsigned char *indiv, const bcfgpu_bcf_key *jobs, const int32_t *col,
                                                                    const bcfgpu_call_site *site, int n_smpl_in, int n_smpl,
                                                                    const unsigned long long *off, const uint32_t *word, unsigned char *buf)
{
    __shared__ __attribute__((aligned(16))) unsigned char in_stage[KENC_LINE + KENC_SLICE], out_stage[KENC_LINE + KENC_SLICE];
    const int j = blockIdx.x, tid = threadIdx.x;
    if (off[j + 1] == off[j]) return;                                       // no record at this job's site
    const bcfgpu_bcf_key J = jobs[j];
    const KeyJob K = kenc_job(indiv, J, site[J.site]);
    const uint32_t wd = word[j];
    const int t = (int)(wd & 3u), es = t == 3 ? 4 : t, w = (int)(wd >> 2), id = J.key_id;
    unsigned char *dst = buf + off[j];
    if (tid == 0) {                                                         // typed key id, then the type / length descriptor
        unsigned char *h = dst;
        if (id <= 127) { h[0] = 0x11; h[1] = (unsigned char)id; h += 2; }
        else if (id <= 32767) { h[0] = 0x12; h[1] = (unsigned char)(id & 0xff); h[2] = (unsigned char)(id >> 8); h += 3; }
        else { h[0] = 0x13; h[1] = (unsigned char)(id & 0xff); h[2] = (unsigned char)(id >> 8 & 0xff); h[3] = (unsigned char)(id >> 16 & 0xff); h[4] = (unsigned char)(id >> 24 & 0xff); h += 5; }
        if (w < 15) h[0] = (unsigned char)(w << 4 | t);
        else if (w <= 127) { h[0] = (unsigned char)(0xF0 | t); h[1] = 0x11; h[2] = (unsigned char)w; }
        else { h[0] = (unsigned char)(0xF0 | t); h[1] = 0x12; h[2] = (unsigned char)(w & 0xff); h[3] = (unsigned char)(w >> 8); }
    }
    dst += kenc_id_bytes(id) + kenc_desc_bytes(w);
    const int per_o = w * es, per_i = K.width * K.es;                       // bytes a sample in the record, in the input (0: no values)
    const int slice_o = KENC_SLICE / per_o, slice_i = per_i ? KENC_SLICE / per_i : n_smpl_in;
    // without a sample map a slice of called samples is the same slice of input samples; with one, the whole run stays in the
    // stage when it fits, else every input slice passes once per output slice
    const int slice = col ? slice_o : slice_o < slice_i ? slice_o : slice_i;
    const bool whole = col && per_i && n_smpl_in <= slice_i;
    const unsigned char *l_in = in_stage;
    if (whole) { l_in = in_stage + kenc_stage(in_stage, K.run, n_smpl_in * per_i, tid); __syncthreads(); }
    for (int s0 = 0; s0 < n_smpl; s0 += slice) {
        const int cs = n_smpl - s0 < slice ? n_smpl - s0 : slice, nb = cs * per_o;
        unsigned char *g = dst + (size_t)s0 * per_o;                        // where the slice's first byte goes
        const int sh = (int)((uintptr_t)g & (KENC_LINE - 1));
        unsigned char *l = out_stage + sh;
        const bool bytewise = sh % es != 0;                                 // values that straddle their natural alignment: byte by byte
        // Lanes read `per_i` and write `per_o` bytes apart.  By the bank rule (32 banks of 4 bytes for ds_read_b32 and narrower and
        // for every write, lanes in groups of 32) a sample of d dwords is gcd(d, 32)-way: an int32 AD of 3 or 5 alleles, and any odd
        // number of dwords, is free of conflicts, 2, 4 and 6 dwords 2-, 4- and 2-way; below 4 bytes a sample (DP, SP, an int8 AD)
        // neighbouring lanes share a dword: reads broadcast, writes to one dword from several lanes are as many stores; not measured
        #define KENC_PUT(P, S) do { if (bytewise) kenc_put_sample<true>(K, (P), w, es, l + (size_t)(S) * per_o); \
                                    else kenc_put_sample<false>(K, (P), w, es, l + (size_t)(S) * per_o); } while (0)
        if (!per_i) {
            for (int s = tid; s < cs; s += KENC_THREADS) KENC_PUT(nullptr, s);
        } else if (!col) {
            l_in = in_stage + kenc_stage(in_stage, K.run + (size_t)s0 * per_i, cs * per_i, tid);
            __syncthreads();
            for (int s = tid; s < cs; s += KENC_THREADS) KENC_PUT(l_in + (size_t)s * per_i, s);
        } else if (whole) {
            for (int s = tid; s < cs; s += KENC_THREADS) KENC_PUT(l_in + (size_t)col[s0 + s] * per_i, s);
        } else {
            for (int i0 = 0; i0 < n_smpl_in; i0 += slice_i) {
                const int ci = n_smpl_in - i0 < slice_i ? n_smpl_in - i0 : slice_i;
                l_in = in_stage + kenc_stage(in_stage, K.run + (size_t)i0 * per_i, ci * per_i, tid);
                __syncthreads();
                for (int s = tid; s < cs; s += KENC_THREADS) {
                    const int c = col[s0 + s] - i0;
                    if (c >= 0 && c < ci) KENC_PUT(l_in + (size_t)c * per_i, s);
                }
                __syncthreads();
            }
        }
        #undef KENC_PUT
        __syncthreads();
        // LDS bytes [sh, sh + nb) -> g - sh + the same offsets: whole 16-byte lines in the middle, single bytes at both ends
        const int lo = sh, hi = sh + nb;
        const int l0 = (lo + KENC_LINE - 1) / KENC_LINE, l1 = hi / KENC_LINE;   // whole lines [l0, l1)
        unsigned char *ga = g - sh;
        if (l0 < l1) {
            for (int x = l0 + tid; x < l1; x += KENC_THREADS)
                reinterpret_cast<uint4*>(ga)[x] = reinterpret_cast<const uint4*>(out_stage)[x];
            const int head = l0 * KENC_LINE - lo, tail = hi - l1 * KENC_LINE;   // each < 16
            if (tid < head) ga[lo + tid] = out_stage[lo + tid];
            else if (tid >= 32 && tid - 32 < tail) ga[l1 * KENC_LINE + tid - 32] = out_stage[l1 * KENC_LINE + tid - 32];
        } else {
            for (int x = lo + tid; x < hi; x += KENC_THREADS) ga[x] = out_stage[x];  // fewer than 31 bytes, no whole line
        }
        __syncthreads();
    }
}

}  // namespace bcfgpu

extern "C" int bcfgpu_call_remap_bcf(bcfgpu_ctx *ctx, int32_t n_keys, const bcfgpu_bcf_key *keys, int32_t n_smpl_in, const void *d_indiv,
                                     uint64_t n_indiv_bytes, const int32_t *col, const bcfgpu_call_site *d_site, int32_t n_sites, const uint8_t *d_emit,
                                     void *d_buf, uint64_t cap_bytes, uint64_t *d_off, uint64_t *n_bytes)
{
    if (!n_bytes) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_remap_bcf: bad arguments");
    *n_bytes = 0;
    if (!ctx || !d_off || n_keys < 0 || n_sites < 0 || n_smpl_in < 1 || (cap_bytes && !d_buf) || (n_indiv_bytes && !d_indiv) || (n_keys && (!keys || !d_site)))
        return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_remap_bcf: bad arguments");
    if ((uint64_t)n_keys + 1 > (uint64_t)INT32_MAX) return bcfgpu_set_error(BCFGPU_E_RANGE, "bcfgpu_call_remap_bcf: too many keys for one call");
    hipStream_t st;
    if (bcfgpu_internal_device(ctx, &st, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_remap_bcf: bad context");
    const int S = bcfgpu_internal_cfg(ctx)->n_smpl;
    if (S < 1 || (!col && S > n_smpl_in)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_remap_bcf: more called samples than input samples and no sample map");
    if (col) for (int s = 0; s < S; ++s) if (col[s] < 0 || col[s] >= n_smpl_in) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_remap_bcf: a sample map entry outside the input samples");
    for (int j = 0; j < n_keys; ++j) {
        const bcfgpu_bcf_key &k = keys[j];
        if (k.type < 0 || k.type > 3 || k.width < 0 || k.width > BCFGPU_BCF_KEY_MAX_WIDTH) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_remap_bcf: a key's type is not 0-3 or its width not 0-255");
        if (k.site < 0 || k.site >= n_sites || k.key_id < 0) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_remap_bcf: a key's site is outside the sites or its id negative");
        if ((k.flags & 1) && (k.nals < 1 || k.nals > BCFGPU_MAX_ALLELES)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_remap_bcf: a Number=R key of a record with no or more than 5 alleles");
    }
    for (int j = 0; j < n_keys; ++j) {
        if (!keys[j].type || !keys[j].width) continue;
        const uint64_t bytes = (uint64_t)n_smpl_in * (uint64_t)keys[j].width * (keys[j].type == 3 ? 4u : (unsigned)keys[j].type);      // < 2^64
        if (bytes > n_indiv_bytes || keys[j].off > n_indiv_bytes - bytes) return bcfgpu_set_error(BCFGPU_E_RANGE, "bcfgpu_call_remap_bcf: a key's values run past the end of the bytes");
    }
    if (n_keys == 0) {
        if (hipMemsetAsync(d_off, 0, sizeof(uint64_t), st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_remap_bcf: offsets");
        return 0;
    }
    const int n_off = n_keys + 1;
    const bcfgpu_bcf_key *d_keys = (const bcfgpu_bcf_key*)ws_upload(ctx, WS_COMPACT_BCFKEY_JOBS, keys, (size_t)n_keys * sizeof *keys, 64, st);
    const int32_t *d_col = col ? (const int32_t*)ws_upload(ctx, WS_COMPACT_BCFKEY_COL, col, (size_t)S * 4, 64, st) : nullptr;
    uint32_t *d_word = (uint32_t*)bcfgpu_internal_ws(ctx, WS_COMPACT_BCFKEY_WORD, (size_t)n_keys * 4 + 64);
    uint64_t *h_total = (uint64_t*)bcfgpu_internal_pinned(ctx, PIN_BCFKEY_TOTAL, sizeof(uint64_t));
    if (!d_keys || (col && !d_col) || !d_word || !h_total) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_call_remap_bcf: workspace");
    unsigned long long *off = reinterpret_cast<unsigned long long*>(d_off);
    hipLaunchKernelGGL(keybcf_size_kernel, dim3(n_keys + 1), dim3(KENC_THREADS), 0, st, (const unsigned char*)d_indiv, d_keys, d_col, d_site, d_emit,
                       n_keys, n_smpl_in, S, off, d_word);
    size_t tmp = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, off, off, n_off, st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_remap_bcf: scan");
    void *d_tmp = bcfgpu_internal_ws(ctx, WS_COMPACT_BCFKEY_SCAN_TMP, tmp + 64);
    if (!d_tmp) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_call_remap_bcf: workspace");
    if (hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp, off, off, n_off, st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_remap_bcf: scan");
    if (hipMemcpyAsync(h_total, off + n_off - 1, sizeof(uint64_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_remap_bcf: size pass");
    *n_bytes = *h_total;
    // the blocks do not fit: nothing is written, the caller learns the size and may come back with a larger buffer
    if (*n_bytes > cap_bytes) return bcfgpu_set_error(BCFGPU_E_RANGE, "bcfgpu_call_remap_bcf: the buffer is too small for the blocks (n_bytes tells the size)");
    if (*n_bytes == 0) return 0;
    hipLaunchKernelGGL(keybcf_write_kernel, dim3(n_keys), dim3(KENC_THREADS), 0, st, (const unsigned char*)d_indiv, d_keys, d_col, d_site, n_smpl_in, S, off, d_word,
                       (unsigned char*)d_buf);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_remap_bcf: write pass");
    return 0;
}
