// vcfcallenc.hip -- the sample columns of a call record as VCF text, made on the device: what the text route does per record on one
// host thread -- print_gt and print_sample_text of host/bcfgpu_call.c over the GT, PL and GQ planes that came down, vio_indiv_text
// (host/vcfio.c), the split per sample and key and print_numberR over the input record's bytes; behind them vcf_format of htslib
// vcf.c and mcall.c:1158-1265, :1583, :1618-1623.  Per called sample the record holds a tab, then its fields joined by ':'.  A
// field is one of the caller's planes (bcfcallenc.hip's rules, as text) or a pass-through key read from the input's bytes
// (bcfkeys.hip's vector and remap, as text); the caller lists a site's fields in FORMAT order, so the pass-through keys lie between
// GT, PL and GQ where the record has them -- which is why ready columns of either side cannot simply be joined.
//
//   callvcf_size_kernel   one workgroup a site, a lane a called sample: the length of every sample's text, summed to the site's size
//   enc_offsets           the sites' offsets (the device scan, gather.hip)
//   callvcf_write_kernel  one workgroup a site, a lane a called sample, in rounds of up to 256 samples: the lengths again, their
//                         exclusive scan over the workgroup, then every lane formats its sample into LDS at its offset -- field by
//                         field, each number from its known end backwards -- and the round's bytes are stored from there 16 bytes
//                         a lane, from any byte the block starts at (line_store, bcfcodec.h).  A round ends with the last sample
//                         whose text still lies inside the stage (bytes, not a number of samples).
// The input side: a lane reads its sample's values of a key where they lie in global memory.  A site has up to 16 fields of
// different widths and types; staging each key's slice (line_load, as bcfkeys.hip does for its one key a workgroup) would take a
// second stage, two barriers a field and round, and with a sample map every input slice once per round.  Read in place, the
// lanes of a round touch one contiguous piece of each run (neighbouring lanes neighbouring samples; with a map whatever the map
// says), the same code serves both cases, and the one LDS stage is the text's.
#include <hipcub/hipcub.hpp>
#include <vector>
#include "bcfcodec.h"

using namespace bcfgpu;

static_assert(sizeof(bcfgpu_vcf_field) == 32 && sizeof(bcfgpu_vcf_field) == sizeof(bcfgpu_bcf_key), "bcfgpu_vcf_field is 32 bytes, the layout of bcfgpu_bcf_key");

namespace bcfgpu {

constexpr int CVCF_STAGE = BCFGPU_VCF_SAMPLE_CAP;               // payload bytes of a round in LDS
static_assert(CVCF_STAGE % COD_LINE == 0, "the stage is whole lines");
static_assert(CVCF_STAGE <= COD_SLICE, "with the scan's storage the workgroup's LDS stays below bcfkeys.hip's two stages");
// One sample always fits the stage, so every round takes at least one: the entry refuses a site whose bound (cvcf_field_bound
// summed, below) passes BCFGPU_VCF_SAMPLE_CAP, and sample_text never writes more than that bound.

struct CallVcfArgs {
    const bcfgpu_call_site *site;
    const int8_t *gt;
    const int32_t *pl, *gq;
    int n_gt_max;
    const bcfgpu_vcf_field *fields;     // [n_fields]
    const int32_t *first;               // [n_sites + 1]: site k's fields are first[k] .. first[k + 1] - 1
    const unsigned char *indiv;
    const int32_t *col;                 // [n_smpl] or nullptr
    int n_smpl;
};

// The text of called sample s at site k (fields f0 .. f1 - 1): its length, and with WRITE its bytes at p (LDS).
template <bool WRITE>
__device__ __forceinline__ int sample_text(const CallVcfArgs &A, const bcfgpu_call_site &c, size_t k, int f0, int f1, int s, unsigned char *p)
{
    const size_t S = (size_t)A.n_smpl;
    int len = 0;
    for (int f = f0; f < f1; ++f) {
        const bcfgpu_vcf_field F = A.fields[f];
        if (WRITE) p[len] = f == f0 ? '\t' : ':';
        ++len;
        if (F.kind == BCFGPU_VCF_FIELD_GT) {
            const int g0 = A.gt[(k * 2 + 0) * S + s], g1 = A.gt[(k * 2 + 1) * S + s];
            if (WRITE) p[len] = gt_char(g0);
            ++len;
            if (g1 != BCFGPU_GT_VECTOR_END) {
                if (WRITE) { p[len] = '/'; p[len + 1] = gt_char(g1); }
                len += 2;
            }
        } else if (F.kind == BCFGPU_VCF_FIELD_PL) {
            const int nn = c.nals_new < 1 ? 1 : c.nals_new > BCFGPU_MAX_ALLELES ? BCFGPU_MAX_ALLELES : c.nals_new;
            int ngn = nn * (nn + 1) / 2; if (ngn > A.n_gt_max) ngn = A.n_gt_max;
            const int32_t *q = A.pl + k * A.n_gt_max * S + s;
            int j = 0;
            for (; j < ngn; ++j) {
                const int32_t v = q[(size_t)j * S];
                if (v == BCFGPU_INT32_VECTOR_END) break;
                if (j) { if (WRITE) p[len] = ','; ++len; }
                len += text_value<WRITE>(p + len, v);
            }
            if (j == 0) { if (WRITE) p[len] = '.'; ++len; }
        } else if (F.kind == BCFGPU_VCF_FIELD_GQ) {
            len += text_value<WRITE>(p + len, A.gq[k * S + s]);
        } else {
            const KeyJob K = kenc_job(A.indiv, F, c);
            const unsigned char *q = K.run + (size_t)(A.col ? A.col[s] : s) * (size_t)(K.width * K.es);     // (not read when the key has no values)
            const int n = K.width ? kenc_len(K, q) : 0;
            const bool remap = K.remap && (n < 1 ? 1 : n) == K.nals;
            const int olen = remap ? K.nn : n < 1 ? 1 : n;
            for (int j = 0; j < olen; ++j) {
                const int src = remap ? kenc_src(K, j) : j;
                const int32_t v = src < 0 || n == 0 ? BCFGPU_INT32_MISSING : get_int(q + src * K.es, K.es, K.aligned);
                if (j) { if (WRITE) p[len] = ','; ++len; }
                len += text_value<WRITE>(p + len, v);
            }
        }
    }
    return len;
}

// size[k] = bytes of site k's text (0: no record, no field), size[n_sites] = 0
__global__ __launch_bounds__(COD_THREADS) void callvcf_size_kernel(CallVcfArgs A, const uint8_t *emit, int n_sites, unsigned long long *size)
{
    __shared__ unsigned long long red[COD_THREADS / 64];
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= n_sites) { if (tid == 0) size[n_sites] = 0; return; }
    const int f0 = A.first[k], f1 = A.first[k + 1];
    if (f0 == f1 || (emit && !emit[k])) { if (tid == 0) size[k] = 0; return; }
    const bcfgpu_call_site c = A.site[k];
    unsigned long long b = 0;
    for (int s = tid; s < A.n_smpl; s += COD_THREADS) b += (unsigned long long)sample_text<false>(A, c, (size_t)k, f0, f1, s, nullptr);
    for (int d = 32; d; d >>= 1) b += __shfl_xor(b, d, 64);
    if ((tid & 63) == 0) red[tid >> 6] = b;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < COD_THREADS / 64; ++w) t += red[w];
        size[k] = t;
    }
}

__global__ __launch_bounds__(COD_THREADS) void callvcf_write_kernel(CallVcfArgs A, int n_sites, const unsigned long long *off, unsigned char *buf)
{
    typedef hipcub::BlockScan<int, COD_THREADS> Scan;
    __shared__ __attribute__((aligned(16))) unsigned char stage[COD_LINE + CVCF_STAGE];
    __shared__ typename Scan::TempStorage scan_tmp;
    __shared__ int round_bytes;
    const int k = blockIdx.x, tid = threadIdx.x;
    if (off[k + 1] == off[k]) return;                                       // no record at this site
    const int f0 = A.first[k], f1 = A.first[k + 1], n_smpl = A.n_smpl;
    const bcfgpu_call_site c = A.site[k];
    unsigned char *g = buf + off[k];                                        // where the round's first byte goes
    for (int s0 = 0; s0 < n_smpl; ) {
        // the lengths of up to 256 samples and where each starts in the round; the round ends with the last sample whose text
        // ends inside the stage (the lanes that fit are the first `fit` ones: the ends only grow; lane 0 always fits)
        const int s = s0 + tid;
        const int len = s < n_smpl ? sample_text<false>(A, c, (size_t)k, f0, f1, s, nullptr) : 0;
        int at;
        Scan(scan_tmp).ExclusiveSum(len, at);
        const bool in = s < n_smpl && at + len <= CVCF_STAGE;
        const int fit = __syncthreads_count(in);
        if (fit < 1) return;                                                // (cannot be: the entry's bound; a round that took nothing would not end)
        if (tid == fit - 1) round_bytes = at + len;
        const int sh = line_shift(g);
        // every lane's text into LDS: single bytes at offsets that depend on the values before them (bank conflicts not measured)
        if (in) sample_text<true>(A, c, (size_t)k, f0, f1, s, stage + sh + at);
        __syncthreads();
        const int nb = round_bytes;
        line_store(stage, g, nb, tid);
        __syncthreads();
        g += nb; s0 += fit;
    }
}

// values x (longest text of a value + 1) of one field: its share of the bound on a sample's text (include/bcfgpu.h)
static uint64_t cvcf_field_bound(const bcfgpu_vcf_field &f, int n_gt_max)
{
    switch (f.kind) {
        case BCFGPU_VCF_FIELD_GT: return 4;
        case BCFGPU_VCF_FIELD_PL: return (uint64_t)n_gt_max * 12;
        case BCFGPU_VCF_FIELD_GQ: return 12;
        default: {
            uint64_t values = f.type && f.width > 1 ? (uint64_t)f.width : 1;
            if ((f.flags & 1) && values < BCFGPU_MAX_ALLELES) values = BCFGPU_MAX_ALLELES;
            return values * (f.type == 3 ? 12u : f.type == 2 ? 7u : 5u);
        }
    }
}

}  // namespace bcfgpu

extern "C" int bcfgpu_call_encode_vcf(bcfgpu_ctx *ctx, int32_t n_sites, int32_t n_gt_max, const bcfgpu_call_out *planes,
                                      int32_t n_fields, const bcfgpu_vcf_field *fields,
                                      int32_t n_smpl_in, const void *d_indiv, uint64_t n_indiv_bytes, const int32_t *col,
                                      const uint8_t *d_emit, void *d_buf, uint64_t cap_bytes, uint64_t *d_off, uint64_t *n_bytes)
{
    if (!n_bytes) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_vcf: bad arguments");
    *n_bytes = 0;
    if (!ctx || !planes || !d_off || n_sites < 0 || n_fields < 0 || n_smpl_in < 1 || n_gt_max < 1 || n_gt_max > BCFGPU_MAX_PL || (cap_bytes && !d_buf) ||
        (n_indiv_bytes && !d_indiv) || (n_fields && (!fields || !planes->site)))
        return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_vcf: bad arguments");
    if ((uint64_t)n_sites + 1 > (uint64_t)INT32_MAX) return bcfgpu_set_error(BCFGPU_E_RANGE, "bcfgpu_call_encode_vcf: too many sites for one call");
    hipStream_t st;
    if (bcfgpu_internal_device(ctx, &st, nullptr)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_vcf: bad context");
    const int S = bcfgpu_internal_cfg(ctx)->n_smpl;
    if (S < 1 || (!col && S > n_smpl_in)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_vcf: more called samples than input samples and no sample map");
    if (col) for (int s = 0; s < S; ++s) if (col[s] < 0 || col[s] >= n_smpl_in) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_vcf: a sample map entry outside the input samples");
    // the fields one by one, and each site's range and bound as they pass
    std::vector<int32_t> first((size_t)n_sites + 1, 0);
    uint64_t bound = 1; int n_here = 0;
    for (int j = 0; j < n_fields; ++j) {
        const bcfgpu_vcf_field &f = fields[j];
        if (f.kind < BCFGPU_VCF_FIELD_GT || f.kind > BCFGPU_VCF_FIELD_KEY) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_vcf: a field's kind is none of BCFGPU_VCF_FIELD_*");
        if (f.site < 0 || f.site >= n_sites) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_vcf: a field's site is outside the sites");
        if (j && f.site < fields[j - 1].site) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_vcf: the fields are not ordered by site");
        if (f.kind == BCFGPU_VCF_FIELD_KEY) {
            if (f.type < 0 || f.type > 3 || f.width < 0 || f.width > BCFGPU_BCF_KEY_MAX_WIDTH) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_vcf: a key's type is not 0-3 or its width not 0-255");
            if ((f.flags & 1) && (f.nals < 1 || f.nals > BCFGPU_MAX_ALLELES)) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_vcf: a Number=R key of a record with no or more than 5 alleles");
        } else if (f.kind == BCFGPU_VCF_FIELD_GT ? !planes->gt : f.kind == BCFGPU_VCF_FIELD_PL ? !planes->pl : !planes->gq)
            return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_vcf: GT, PL or GQ is listed and its plane is NULL");
        if (j == 0 || f.site != fields[j - 1].site) { bound = 1; n_here = 0; }
        if (++n_here > BCFGPU_VCF_MAX_FIELDS) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_vcf: more than 16 fields at a site");
        bound += cvcf_field_bound(f, n_gt_max);
        if (bound > BCFGPU_VCF_SAMPLE_CAP) return bcfgpu_set_error(BCFGPU_E_ARG, "bcfgpu_call_encode_vcf: a sample's text at a site may pass BCFGPU_VCF_SAMPLE_CAP");
        first[(size_t)f.site + 1] = j + 1;
    }
    for (int j = 0; j < n_fields; ++j) {
        const bcfgpu_vcf_field &f = fields[j];
        if (f.kind != BCFGPU_VCF_FIELD_KEY || !f.type || !f.width) continue;
        const uint64_t bytes = (uint64_t)n_smpl_in * (uint64_t)f.width * (f.type == 3 ? 4u : (unsigned)f.type);      // < 2^64
        if (bytes > n_indiv_bytes || f.off > n_indiv_bytes - bytes) return bcfgpu_set_error(BCFGPU_E_RANGE, "bcfgpu_call_encode_vcf: a key's values run past the end of the bytes");
    }
    if (n_sites == 0) return enc_offsets(ctx, st, "bcfgpu_call_encode_vcf", d_off, 1, cap_bytes, n_bytes);
    for (int k = 0; k < n_sites; ++k) if (first[(size_t)k + 1] < first[k]) first[(size_t)k + 1] = first[k];    // a site without a field: an empty range
    CallVcfArgs A;
    A.site = planes->site; A.gt = planes->gt; A.pl = planes->pl; A.gq = planes->gq; A.n_gt_max = n_gt_max;
    A.fields = (const bcfgpu_vcf_field*)ws_upload(ctx, WS_COMPACT_CALLVCF_FIELDS, fields, (size_t)n_fields * sizeof *fields, 64, st);
    A.first = (const int32_t*)ws_upload(ctx, WS_COMPACT_CALLVCF_FIRST, first.data(), first.size() * 4, 64, st);
    A.col = col ? (const int32_t*)ws_upload(ctx, WS_COMPACT_CALLVCF_COL, col, (size_t)S * 4, 64, st) : nullptr;
    A.indiv = (const unsigned char*)d_indiv; A.n_smpl = S;
    if (!A.fields || !A.first || (col && !A.col)) { (void)hipStreamSynchronize(st); return bcfgpu_set_error(BCFGPU_E_NOMEM, "bcfgpu_call_encode_vcf: workspace"); }
    unsigned long long *off = reinterpret_cast<unsigned long long*>(d_off);
    hipLaunchKernelGGL(callvcf_size_kernel, dim3(n_sites + 1), dim3(COD_THREADS), 0, st, A, d_emit, n_sites, off);
    const int rc = enc_offsets(ctx, st, "bcfgpu_call_encode_vcf", d_off, n_sites + 1, cap_bytes, n_bytes);
    if (rc || *n_bytes == 0) { (void)hipStreamSynchronize(st); return rc; }       // (`first` is read by its copy until the stream is through)
    hipLaunchKernelGGL(callvcf_write_kernel, dim3(n_sites), dim3(COD_THREADS), 0, st, A, n_sites, off, (unsigned char*)d_buf);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return bcfgpu_set_error(BCFGPU_E_HIP, "bcfgpu_call_encode_vcf: write pass");
    return 0;
}
