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
//   keybcf_size_kernel   one workgroup a key job: the input run in slices of samples through the LDS stage (line_load); per called
//                        sample the output vector's length, largest value and largest negated value (wavefront shuffles, then
//                        LDS) -> the block's width, type and size, one packed word a job
//   enc_offsets          the blocks' offsets (the device scan, gather.hip)
//   keybcf_write_kernel  one workgroup a key job: the header bytes, then the values in slices of called samples -- the input slice
//                        into one LDS stage (line_load, bcfcodec.h), a lane a called sample: its vector out of that stage,
//                        transformed, into a second stage at its place in the record; from there 16 bytes a lane to consecutive
//                        addresses (line_store).
//                        With a sample map the called samples take their sample from the input stage: one load when the whole run
//                        fits a slice, else every input slice once per output slice.
// No straight copy of runs that come out as they went in: every block goes through the transform.
#include "bcfcodec.h"

using namespace bcfgpu;

static_assert(sizeof(bcfgpu_bcf_key) == 32, "bcfgpu_bcf_key is 32 bytes");

namespace bcfgpu {

constexpr int KENC_NRED = 3;                                    // width, max, -min

static_assert(BCFGPU_BCF_KEY_MAX_WIDTH * 4 <= COD_SLICE, "a sample of the widest key fits a slice: a slice is at least 15 samples");

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
            const int32_t v = get_int(p + K.inv[t] * K.es, K.es, K.aligned);
            if (!is_sentinel(v)) { m[1] = v > m[1] ? v : m[1]; m[2] = -v > m[2] ? -v : m[2]; }
        }
    } else {
        for (int j = 0; j < len; ++j) {
            const int32_t v = get_int(p + j * K.es, K.es, K.aligned);
            if (!is_sentinel(v)) { m[1] = v > m[1] ? v : m[1]; m[2] = -v > m[2] ? -v : m[2]; }
        }
    }
    m[0] = olen > m[0] ? olen : m[0];
}

// size[j] = bytes of job j's block (0: its site has no record), size[n_keys] = 0; word[j] = type | width << 2
__global__ __launch_bounds__(COD_THREADS) void keybcf_size_kernel(const unsigned char *indiv, const bcfgpu_bcf_key *jobs, const int32_t *col,
                                                                   const bcfgpu_call_site *site, const uint8_t *emit, int n_keys, int n_smpl_in, int n_smpl,
                                                                   unsigned long long *size, uint32_t *word)
{
    __shared__ __attribute__((aligned(16))) unsigned char stage[COD_LINE + COD_SLICE];
    __shared__ int32_t red[COD_THREADS / 64][KENC_NRED];
    const int j = blockIdx.x, tid = threadIdx.x;
    if (j >= n_keys) { if (tid == 0) size[n_keys] = 0; return; }
    const bcfgpu_bcf_key J = jobs[j];
    if (emit && !emit[J.site]) { if (tid == 0) { size[j] = 0; word[j] = 0; } return; }
    const KeyJob K = kenc_job(indiv, J, site[J.site]);
    int32_t m[KENC_NRED] = { 1, COD_NONE, COD_NONE };
    const int per = K.width * K.es;                                         // bytes an input sample
    if (per) {
        const int slice = COD_SLICE / per;                                 // input samples a slice
        for (int i0 = 0; i0 < n_smpl_in; i0 += slice) {
            if (!col && i0 >= n_smpl) break;                                // the input samples past the called ones
            const int ci = n_smpl_in - i0 < slice ? n_smpl_in - i0 : slice;
            const unsigned char *l = stage + line_load(stage, K.run + (size_t)i0 * per, ci * per, tid);
            __syncthreads();
            if (col) {
                for (int s = tid; s < n_smpl; s += COD_THREADS) {
                    const int c = col[s] - i0;
                    if (c >= 0 && c < ci) kenc_measure(K, l + (size_t)c * per, m);
                }
            } else {
                const int ce = i0 + ci < n_smpl ? ci : n_smpl - i0;
                for (int c = tid; c < ce; c += COD_THREADS) kenc_measure(K, l + (size_t)c * per, m);
            }
            __syncthreads();
        }
    }                                                                       // no values: every sample is one `missing`, m as it starts
    wg_max(m, red, tid);
    if (tid == 0) {
        int w = m[0];
        if (K.remap && per == 0 && K.nals == 1) w = K.nn;                   // ('.' is one value: at one allele it follows the alleles too)
        const int t = int_type(m[1], m[2]);
        size[j] = (unsigned long long)(id_bytes(J.key_id) + desc_bytes(w)) + (unsigned long long)n_smpl * (unsigned)w * (unsigned)elem_bytes(t);
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
            const int src = remap ? kenc_src(K, j) : j;                     // the input value that goes here, -1: `missing`
            x = src < 0 || len == 0 ? BCFGPU_INT32_MISSING : get_int(p + src * K.es, K.es, K.aligned);
        }
        put_int<BYTEWISE>(q + j * es, narrow(x, es), es);
    }
}

__global__ __launch_bounds__(COD_THREADS) void keybcf_write_kernel(const unsigned char *indiv, const bcfgpu_bcf_key *jobs, const int32_t *col,
                                                                    const bcfgpu_call_site *site, int n_smpl_in, int n_smpl,
                                                                    const unsigned long long *off, const uint32_t *word, unsigned char *buf)
{
    __shared__ __attribute__((aligned(16))) unsigned char in_stage[COD_LINE + COD_SLICE], out_stage[COD_LINE + COD_SLICE];
    const int j = blockIdx.x, tid = threadIdx.x;
    if (off[j + 1] == off[j]) return;                                       // no record at this job's site
    const bcfgpu_bcf_key J = jobs[j];
    const KeyJob K = kenc_job(indiv, J, site[J.site]);
    const uint32_t wd = word[j];
    const int t = (int)(wd & 3u), es = elem_bytes(t), w = (int)(wd >> 2), id = J.key_id;
    unsigned char *dst = buf + off[j];
    if (tid == 0) put_header(dst, id, w, t);
    dst += id_bytes(id) + desc_bytes(w);
    const int per_o = w * es, per_i = K.width * K.es;                       // bytes a sample in the record, in the input (0: no values)
    const int slice_o = COD_SLICE / per_o, slice_i = per_i ? COD_SLICE / per_i : n_smpl_in;
    // without a sample map a slice of called samples is the same slice of input samples; with one, the whole run stays in the
    // stage when it fits, else every input slice passes once per output slice
    const int slice = col ? slice_o : slice_o < slice_i ? slice_o : slice_i;
    const bool whole = col && per_i && n_smpl_in <= slice_i;
    const unsigned char *l_in = in_stage;
    if (whole) { l_in = in_stage + line_load(in_stage, K.run, n_smpl_in * per_i, tid); __syncthreads(); }
    for (int s0 = 0; s0 < n_smpl; s0 += slice) {
        const int cs = n_smpl - s0 < slice ? n_smpl - s0 : slice, nb = cs * per_o;
        unsigned char *g = dst + (size_t)s0 * per_o;                        // where the slice's first byte goes
        const int sh = line_shift(g);
        unsigned char *l = out_stage + sh;
        const bool bytewise = sh % es != 0;                                 // values that straddle their natural alignment: byte by byte
        // Lanes read `per_i` and write `per_o` bytes apart.  By the bank rule (32 banks of 4 bytes for ds_read_b32 and narrower and
        // for every write, lanes in groups of 32) a sample of d dwords is gcd(d, 32)-way: an int32 AD of 3 or 5 alleles, and any odd
        // number of dwords, is free of conflicts, 2, 4 and 6 dwords 2-, 4- and 2-way; below 4 bytes a sample (DP, SP, an int8 AD)
        // neighbouring lanes share a dword: reads broadcast, writes to one dword from several lanes are as many stores; not measured
        auto put = [&](const unsigned char *p, int s) { if (bytewise) kenc_put_sample<true>(K, p, w, es, l + (size_t)s * per_o);
                                                        else kenc_put_sample<false>(K, p, w, es, l + (size_t)s * per_o); };
        if (!per_i) {
            for (int s = tid; s < cs; s += COD_THREADS) put(nullptr, s);
        } else if (!col) {
            l_in = in_stage + line_load(in_stage, K.run + (size_t)s0 * per_i, cs * per_i, tid);
            __syncthreads();
            for (int s = tid; s < cs; s += COD_THREADS) put(l_in + (size_t)s * per_i, s);
        } else if (whole) {
            for (int s = tid; s < cs; s += COD_THREADS) put(l_in + (size_t)col[s0 + s] * per_i, s);
        } else {
            for (int i0 = 0; i0 < n_smpl_in; i0 += slice_i) {
                const int ci = n_smpl_in - i0 < slice_i ? n_smpl_in - i0 : slice_i;
                l_in = in_stage + line_load(in_stage, K.run + (size_t)i0 * per_i, ci * per_i, tid);
                __syncthreads();
                for (int s = tid; s < cs; s += COD_THREADS) {
                    const int c = col[s0 + s] - i0;
                    if (c >= 0 && c < ci) put(l_in + (size_t)c * per_i, s);
                }
                __syncthreads();
            }
        }
        __syncthreads();
        line_store(out_stage, g, nb, tid);
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
    if (n_keys == 0) return enc_offsets(ctx, st, "bcfgpu_call_remap_bcf", d_off, 1, cap_bytes, n_bytes);
    const int n_off = n_keys + 1;
    const bcfgpu_bcf_key *d_keys = (const bcfgpu_bcf_key*)ws_upload(ctx, WS_COMPACT_BCFKEY_JOBS, keys, (size_t)n_keys * sizeof *keys, 64, st);
    const int32_t *d_col = col ? (const int32_t*)ws_upload(ctx, WS_COMPACT_BCFKEY_COL, col, (size_t)S * 4, 64, st) : nullptr;
    uint32_t *d_word = (uint32_t*)bcfgpu_internal_ws(ctx, WS_COMPACT_BCFKEY_WORD, (size_t)n_keys * 4 + 64);
    if (!d_keys || (col && !d_col) || !d_word) return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_call_remap_bcf: workspace");
    unsigned long long *off = reinterpret_cast<unsigned long long*>(d_off);
    hipLaunchKernelGGL(keybcf_size_kernel, dim3(n_keys + 1), dim3(COD_THREADS), 0, st, (const unsigned char*)d_indiv, d_keys, d_col, d_site, d_emit,
                       n_keys, n_smpl_in, S, off, d_word);
    const int rc = enc_offsets(ctx, st, "bcfgpu_call_remap_bcf", d_off, n_off, cap_bytes, n_bytes);
    if (rc || *n_bytes == 0) return rc;
    hipLaunchKernelGGL(keybcf_write_kernel, dim3(n_keys), dim3(COD_THREADS), 0, st, (const unsigned char*)d_indiv, d_keys, d_col, d_site, n_smpl_in, S, off, d_word,
                       (unsigned char*)d_buf);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_remap_bcf: write pass");
    return 0;
}
