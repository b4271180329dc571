// bcfcodec.h -- what the device codecs of the records' per-sample bytes have in common (bcfenc.hip, vcfenc.hip, bcfcallenc.hip,
// bcfkeys.hip, bcfdec.hip, vcfcallenc.hip, vcfdec.hip, vcfcallrw.hip, vcfkeys.hip): the line-wise copy between global memory and the LDS stage, the BCF2 block
// header and typed-value rules (bcf_enc_vint / bcf_dec_int of htslib vcf.c; here host/vcfio.c enc_int1 / enc_size / enc_vint /
// dec_int), the workgroup maximum of the size kernels, decimal text written and read, the reading of a pass-through key from the
// input's bytes, and the FORMAT keys of an mpileup record.  Device and host-inline code only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "ctx.h"

namespace bcfgpu {

constexpr int COD_THREADS = 256;
constexpr int COD_LINE = 16;                                    // bytes a lane loads / stores at once
constexpr int COD_SLICE = BCFGPU_MAX_PL * 4 * 256;              // payload bytes of a slice in LDS: 256 samples of the widest PL as int32

// ---- the line copy ----
// A stage is COD_LINE + payload bytes of LDS, 16-byte aligned.  A run of nb bytes at global address g (any alignment) has its place
// in the stage at sh = g mod 16, so that the aligned 16-byte lines of both coincide.
__device__ __forceinline__ int line_shift(const unsigned char *g) { return (int)((uintptr_t)g & (COD_LINE - 1)); }

// bytes [lo, hi) of src -> the same offsets of dst (both 16-byte aligned, one of them the stage): whole lines in the middle, a lane
// a line, consecutive lanes consecutive lines; the bytes before the first whole line from lanes 0..15, those after the last from
// lanes 32..47.  No byte outside [lo, hi) is read or written.  The caller synchronises.
__device__ __forceinline__ void line_copy(unsigned char *dst, const unsigned char *src, int lo, int hi, int tid)
{
    const int l0 = (lo + COD_LINE - 1) / COD_LINE, l1 = hi / COD_LINE;      // whole lines [l0, l1)
    if (l0 < l1) {
        for (int x = l0 + tid; x < l1; x += COD_THREADS)
            reinterpret_cast<uint4*>(dst)[x] = reinterpret_cast<const uint4*>(src)[x];
        const int head = l0 * COD_LINE - lo, tail = hi - l1 * COD_LINE;     // each < 16
        if (tid < head) dst[lo + tid] = src[lo + tid];
        else if (tid >= 32 && tid - 32 < tail) dst[l1 * COD_LINE + tid - 32] = src[l1 * COD_LINE + tid - 32];
    } else {
        for (int x = lo + tid; x < hi; x += COD_THREADS) dst[x] = src[x];   // fewer than 31 bytes, no whole line
    }
}
// global bytes g[0, nb) -> stage[sh, sh + nb), and stage[sh, sh + nb) -> g[0, nb); both return sh
__device__ __forceinline__ int line_load(unsigned char *stage, const unsigned char *g, int nb, int tid)
{
    const int sh = line_shift(g);
    line_copy(stage, g - sh, sh, sh + nb, tid);
    return sh;
}
__device__ __forceinline__ int line_store(const unsigned char *stage, unsigned char *g, int nb, int tid)
{
    const int sh = line_shift(g);
    line_copy(g - sh, stage, sh, sh + nb, tid);
    return sh;
}

// ---- a key's block: typed key id, type / length descriptor, then n_smpl x w integers of type t ----
__device__ __forceinline__ int id_bytes(int id) { return id <= 127 ? 2 : id <= 32767 ? 3 : 5; }          // a typed scalar: descriptor + value
// width >= 15: 0xF?, then the width as a typed int8 / int16.  Only bcfkeys.hip passes widths on (up to BCFGPU_BCF_KEY_MAX_WIDTH); the
// widths bcfenc.hip and bcfcallenc.hip make are at most BCFGPU_MAX_PL, so they never take the int16 form
__device__ __forceinline__ int desc_bytes(int w) { return w < 15 ? 1 : w <= 127 ? 3 : 4; }
static_assert(BCFGPU_MAX_PL <= 127 && BCFGPU_MAX_ALLELES <= 127 && BCFGPU_MAX_ALLELES * (BCFGPU_MAX_ALLELES + 1) / 2 <= BCFGPU_MAX_PL,
              "an mpileup or call key is at most BCFGPU_MAX_PL values wide: its width is a typed int8");
__device__ __forceinline__ int elem_bytes(int t) { return t == 3 ? 4 : t; }

// the id_bytes(id) + desc_bytes(w) bytes in front of the values
__device__ __forceinline__ void put_header(unsigned char *h, int id, int w, int t)
{
    if (id <= 127) { h[0] = 0x11; h[1] = (unsigned char)id; h += 2; }
    else if (id <= 32767) { h[0] = 0x12; h[1] = (unsigned char)(id & 0xff); h[2] = (unsigned char)(id >> 8); h += 3; }
    else { h[0] = 0x13; h[1] = (unsigned char)(id & 0xff); h[2] = (unsigned char)(id >> 8 & 0xff); h[3] = (unsigned char)(id >> 16 & 0xff); h[4] = (unsigned char)(id >> 24 & 0xff); h += 5; }
    if (w < 15) h[0] = (unsigned char)(w << 4 | t);
    else if (w <= 127) { h[0] = (unsigned char)(0xF0 | t); h[1] = 0x11; h[2] = (unsigned char)w; }
    else { h[0] = (unsigned char)(0xF0 | t); h[1] = 0x12; h[2] = (unsigned char)(w & 0xff); h[3] = (unsigned char)(w >> 8); }
}

// ---- typed values ----
constexpr int32_t COD_NONE = INT32_MIN + 1;                     // "no value yet" of a maximum (enc_vint starts there)
__device__ __forceinline__ bool is_sentinel(int32_t v) { return v == BCFGPU_INT32_MISSING || v == BCFGPU_INT32_VECTOR_END; }
// the smallest type for values up to mx and down to -neg_mn (enc_vint's rule: int8 holds -120 .. 127, int16 -32760 .. 32767)
__device__ __forceinline__ int int_type(int32_t mx, int32_t neg_mn) { return mx <= 127 && neg_mn <= 120 ? 1 : mx <= 32767 && neg_mn <= 32760 ? 2 : 3; }

// one value of `es` bytes at q, widened (dec_int: the smallest two values of int8 and int16 are `missing` and `end of vector`)
__device__ __forceinline__ int32_t get_int(const unsigned char *q, int es, bool aligned)
{
    if (es == 1) { const int32_t v = (int8_t)*q; return v == -128 ? BCFGPU_INT32_MISSING : v == -127 ? BCFGPU_INT32_VECTOR_END : v; }
    if (es == 2) {
        const int32_t v = aligned ? (int32_t)*reinterpret_cast<const int16_t*>(q) : (int32_t)(int16_t)(uint16_t)(q[0] | q[1] << 8);
        return v == -32768 ? BCFGPU_INT32_MISSING : v == -32767 ? BCFGPU_INT32_VECTOR_END : v;
    }
    if (aligned) return *reinterpret_cast<const int32_t*>(q);
    return (int32_t)((uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24);
}
// a value as the integer of `es` bytes that stands for it: the sentinels are the type's own, not the int32's low bytes
__device__ __forceinline__ uint32_t narrow(int32_t v, int es)
{
    if (es == 4 || !is_sentinel(v)) return (uint32_t)v;
    return (es == 1 ? 0x80u : 0x8000u) | (uint32_t)(v == BCFGPU_INT32_VECTOR_END);
}
// the low `es` bytes of v at o: one store when o is a multiple of es, else (BYTEWISE) byte by byte
template <bool BYTEWISE>
__device__ __forceinline__ void put_int(unsigned char *o, uint32_t v, int es)
{
    if (BYTEWISE) { for (int b = 0; b < es; ++b) o[b] = (unsigned char)(v >> (8 * b)); }
    else if (es == 1) *o = (unsigned char)v;
    else if (es == 2) *reinterpret_cast<uint16_t*>(o) = (uint16_t)v;
    else *reinterpret_cast<uint32_t*>(o) = v;
}

// the workgroup's maxima of m[0 .. N), left in thread 0's m: wavefront shuffles, then LDS.  Every thread of the workgroup calls it.
template <int N>
__device__ __forceinline__ void wg_max(int32_t (&m)[N], int32_t (&red)[COD_THREADS / 64][N], int tid)
{
    #pragma unroll
    for (int i = 0; i < N; ++i)
        for (int d = 32; d; d >>= 1) { const int32_t o = __shfl_xor(m[i], d, 64); m[i] = o > m[i] ? o : m[i]; }
    if ((tid & 63) == 0) {
        #pragma unroll
        for (int i = 0; i < N; ++i) red[tid >> 6][i] = m[i];
    }
    __syncthreads();
    if (tid == 0) {
        #pragma unroll
        for (int i = 0; i < N; ++i)
            for (int w = 1; w < COD_THREADS / 64; ++w) m[i] = red[w][i] > m[i] ? red[w][i] : m[i];
    }
}

// ---- decimal text (vcfenc.hip, vcfcallenc.hip) ----
// decimal digits of v, by comparisons
__device__ __forceinline__ int n_digits(uint32_t v)
{
    return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u)
             + (v >= 100000000u) + (v >= 1000000000u);
}
// v in decimal at p (LDS), written from its known end backwards; returns the byte after it
__device__ __forceinline__ unsigned char *put_value(unsigned char *p, uint32_t v)
{
    const int nd = n_digits(v);
    for (int i = nd - 1; i > 0; --i) { const uint32_t q = v / 10u; p[i] = (unsigned char)('0' + (v - q * 10u)); v = q; }
    p[0] = (unsigned char)('0' + v);
    return p + nd;
}
// the signed form: a '-' in front of a negative value's digits
__device__ __forceinline__ int signed_len(int32_t v) { return v < 0 ? 1 + n_digits(0u - (uint32_t)v) : n_digits((uint32_t)v); }
__device__ __forceinline__ unsigned char *put_signed(unsigned char *p, int32_t v)
{
    if (v < 0) { *p++ = '-'; return put_value(p, 0u - (uint32_t)v); }
    return put_value(p, (uint32_t)v);
}
// one value of a text field: '.' for `missing`, else in decimal with its sign; the bytes it takes (vcfcallenc.hip, vcfcallrw.hip)
template <bool WRITE>
__device__ __forceinline__ int text_value(unsigned char *p, int32_t v)
{
    if (v == BCFGPU_INT32_MISSING) { if (WRITE) *p = '.'; return 1; }
    if (WRITE) put_signed(p, v);
    return signed_len(v);
}
// one GT entry: an allele index as its digit, anything else '.'
__device__ __forceinline__ unsigned char gt_char(int g) { return g >= 0 && g <= 9 ? (unsigned char)('0' + g) : (unsigned char)'.'; }

// ---- reading text (vcfdec.hip, vcfcallrw.hip, vcfkeys.hip) ----
constexpr uint32_t VDEC_NO_ERROR = 0xffffffffu;                 // an error word of the indexing pass nobody has touched; else the smallest site at fault
// bit i of the result: byte i of the 16-byte line w is c (the exact zero-byte test on w ^ cccc, then the four high bits of a word
// gathered by one multiplication whose partial products meet on no bit)
__device__ __forceinline__ uint32_t line_match(uint4 w, unsigned char c)
{
    const uint32_t cc = 0x01010101u * c, x[4] = { w.x ^ cc, w.y ^ cc, w.z ^ cc, w.w ^ cc };
    uint32_t m = 0;
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t t = ~(((x[i] & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x[i] | 0x7f7f7f7fu);      // 0x80 in every byte of x[i] that is 0
        m |= (((t >> 7) * 0x00204081u) >> 21 & 0xfu) << (4 * i);
    }
    return m;
}
// bits [lo, hi) of a 16-bit mask, clipped to it
__device__ __forceinline__ uint32_t bit_range(int lo, int hi)
{
    lo = lo < 0 ? 0 : lo; hi = hi > 16 ? 16 : hi;
    return lo < hi ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}
// One value of a FORMAT field: p[i .. n) starts with it, and it ends at ',' (more follow), ':' or n.  '.' alone is `missing`, anything
// else must be [+-]?[0-9]+ inside int32 (the sum saturates far above it, so that leading zeros cost nothing and the test is exact).
// i moves behind the value; false: an empty value, another byte in it, or out of range
__device__ __forceinline__ bool get_text_value(const unsigned char *p, int &i, int n, int32_t &x)
{
    if (i < n && p[i] == '.' && (i + 1 == n || p[i + 1] == ',' || p[i + 1] == ':')) { x = BCFGPU_INT32_MISSING; ++i; return true; }
    bool neg = false;
    if (i < n && (p[i] == '+' || p[i] == '-')) { neg = p[i] == '-'; ++i; }
    unsigned long long a = 0; const int i0 = i;
    for (; i < n; ++i) {
        const unsigned d = (unsigned)p[i] - '0';
        if (d > 9u) break;
        if (a < (1ull << 40)) a = a * 10u + d;
    }
    x = (int32_t)(neg ? 0u - (uint32_t)a : (uint32_t)a);
    return i > i0 && (i == n || p[i] == ',' || p[i] == ':') && a <= (neg ? 2147483648ull : 2147483647ull);
}
// The planes of one called sample from its column's text: p[0] is the tab, the column ends at n.  Field idx (the fields are cut at
// ':') is cut at ','; value j goes to o[j * S] for j < n_planes (the values past them are not looked at), `end of vector` to the planes
// behind the last value; a column with fewer fields, or idx < 0, is '.': `missing`, then `end of vector`.  false: a malformed value
__device__ __forceinline__ bool text_sample(int32_t *o, size_t S, int n_planes, const unsigned char *p, int n, int idx)
{
    int i = 1, f = 0, j = 0;
    bool ok = true;
    for (; f < idx && i < n; ++i) f += p[i] == ':';
    if (idx >= 0 && f == idx) {
        for (;;) {
            int32_t x;
            ok = get_text_value(p, i, n, x);
            o[(size_t)j++ * S] = x;
            if (!ok || j == n_planes || i == n || p[i] != ',') break;
            ++i;
        }
    } else o[(size_t)j++ * S] = BCFGPU_INT32_MISSING;
    for (; j < n_planes; ++j) o[(size_t)j * S] = BCFGPU_INT32_VECTOR_END;
    return ok;
}

// ---- a pass-through key of a call record, read from the input record's bytes (bcfkeys.hip as BCF2, vcfcallenc.hip as text) ----
// what is the same for every sample of a job
struct KeyJob {
    const unsigned char *run;           // value [input sample 0][0]
    int es, width;                      // bytes a value and values a sample in the input (width 0: no values, every sample is '.')
    bool aligned;                       // the run's values lie at their natural alignment
    int nals, nn;                       // alleles of the input record, of the output record
    bool remap;                         // Number=R and alleles dropped: a sample with nals values follows the alleles
    int inv[BCFGPU_MAX_ALLELES];        // output value t is input value inv[t], -1: `missing`
};

// J: a bcfgpu_bcf_key or a bcfgpu_vcf_field of kind KEY (off, type, width, nals, flags)
template <class Job>
__device__ __forceinline__ KeyJob kenc_job(const unsigned char *indiv, const Job &J, const bcfgpu_call_site &c)
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
    for (; len < K.width; ++len) if (get_int(p + len * K.es, K.es, K.aligned) == BCFGPU_INT32_VECTOR_END) break;
    return len;
}

// the input value that goes to place j of a remapped vector, -1: `missing`
__device__ __forceinline__ int kenc_src(const KeyJob &K, int j)
{
    int src = -1;
    #pragma unroll
    for (int t = 0; t < BCFGPU_MAX_ALLELES; ++t) if (t == j) src = K.inv[t];
    return src;
}

// ---- the FORMAT keys of an mpileup record (bcfenc.hip as BCF2, vcfenc.hip as text) ----
struct MplpPlanes {
    const bcfgpu_site *site;
    const uint8_t *pl, *sp;
    const uint16_t *dp4, *adf, *adr, *scr;
    const int32_t *qs;
};
// the keys a record holds, in the order they are written: kind = BCFGPU_BCF_*, id = the writer's dictionary index
struct MplpKeys { int n; int kind[BCFGPU_BCF_NKEYS]; int id[BCFGPU_BCF_NKEYS]; };

__device__ __forceinline__ int key_width(int kind, int na)
{
    switch (kind) {
        case BCFGPU_BCF_PL: return na * (na + 1) / 2;
        case BCFGPU_BCF_DP4: return 4;
        case BCFGPU_BCF_ADF: case BCFGPU_BCF_ADR: case BCFGPU_BCF_AD: case BCFGPU_BCF_DPR: case BCFGPU_BCF_QS: return na;
        default: return 1;                                      // DP, DV, SP, SCR
    }
}

// value j of sample s of the key at site k (bam2bcf.c:845-903: DP and DV are sums of the DP4 counts, AD and DPR of ADF and ADR); never
// negative
__device__ __forceinline__ int32_t key_value(const MplpPlanes &P, int kind, size_t k, int j, int s, size_t S)
{
    switch (kind) {
        case BCFGPU_BCF_PL:  return P.pl[(k * BCFGPU_MAX_PL + j) * S + s];
        case BCFGPU_BCF_DP:  { const uint16_t *d = P.dp4 + k * 4 * S + s; return (int32_t)d[0] + d[S] + d[2 * S] + d[3 * S]; }
        case BCFGPU_BCF_DV:  { const uint16_t *d = P.dp4 + k * 4 * S + s; return (int32_t)d[2 * S] + d[3 * S]; }
        case BCFGPU_BCF_SP:  return P.sp[k * S + s];
        case BCFGPU_BCF_DP4: return P.dp4[(k * 4 + j) * S + s];
        case BCFGPU_BCF_ADF: return P.adf[(k * 5 + j) * S + s];
        case BCFGPU_BCF_ADR: return P.adr[(k * 5 + j) * S + s];
        case BCFGPU_BCF_AD: case BCFGPU_BCF_DPR: return (int32_t)P.adf[(k * 5 + j) * S + s] + P.adr[(k * 5 + j) * S + s];
        case BCFGPU_BCF_SCR: return P.scr[k * S + s];
        default:             return P.qs[(k * 5 + j) * S + s];  // QS (>= 0)
    }
}

__device__ __forceinline__ int site_alleles(const bcfgpu_site &c) { const int na = c.n_alleles; return na < 1 ? 1 : na > BCFGPU_MAX_ALLELES ? BCFGPU_MAX_ALLELES : na; }

// the flag that selects each key, in bcf_call2bcf's order (bam2bcf.c:845-903); PL is always written
constexpr int KEY_FLAG[BCFGPU_BCF_NKEYS] = { 0, BCFGPU_FMT_DP, BCFGPU_FMT_DV, BCFGPU_FMT_SP, BCFGPU_FMT_DP4, BCFGPU_FMT_ADF, BCFGPU_FMT_ADR,
                                             BCFGPU_FMT_AD, BCFGPU_FMT_DPR, BCFGPU_FMT_SCR, BCFGPU_FMT_QS };

// P = the planes; K = the keys cfg->fmt_flag selects, with their ids from key_id (NULL: text, no ids).  0, or the error of entry
// `name`: a negative id, a selected key whose plane is NULL, no site records
inline int mplp_keys(const char *name, const bcfgpu_cfg *cfg, const bcfgpu_mplp_out *planes, const int32_t *key_id, MplpPlanes &P, MplpKeys &K)
{
    P = { planes->site, planes->pl, planes->sp, planes->dp4, planes->adf, planes->adr, planes->scr, planes->qs };
    K.n = 0;
    for (int i = 0; i < BCFGPU_BCF_NKEYS; ++i) {
        if (i != BCFGPU_BCF_PL && !(cfg->fmt_flag & KEY_FLAG[i])) continue;
        if (key_id && key_id[i] < 0) return bcfgpu_set_error(BCFGPU_E_ARG, name, "negative key id");
        K.kind[K.n] = i; K.id[K.n] = key_id ? key_id[i] : 0; ++K.n;
        const bool have = i == BCFGPU_BCF_PL ? P.pl != nullptr : i == BCFGPU_BCF_SP ? P.sp != nullptr : i == BCFGPU_BCF_SCR ? P.scr != nullptr :
                          i == BCFGPU_BCF_QS ? P.qs != nullptr : i == BCFGPU_BCF_ADF ? P.adf != nullptr : i == BCFGPU_BCF_ADR ? P.adr != nullptr :
                          (i == BCFGPU_BCF_AD || i == BCFGPU_BCF_DPR) ? P.adf && P.adr : P.dp4 != nullptr;
        if (!have) return bcfgpu_set_error(BCFGPU_E_ARG, name, "a plane the context's fmt_flag asks for is NULL");
    }
    if (!P.site) return bcfgpu_set_error(BCFGPU_E_ARG, name, "no site records");
    return 0;
}

}  // namespace bcfgpu
