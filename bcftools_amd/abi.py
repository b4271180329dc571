"""ctypes mirror of include/bcfgpu.h (structs, constants, prototypes).

Plain data definitions only; no computation lives here.  Struct field order and
types must match the header exactly (checked by tests/test_abi.py against the
sizes the C library reports).
"""
import ctypes as C

# error codes
OK, E_ARG, E_NOMEM, E_HIP, E_DEPTH, E_NODEV, E_RANGE = 0, -1, -2, -3, -4, -5, -6

# B2B_* (bam2bcf.h:46-62)
FMT_DP, FMT_SP, FMT_DV, FMT_DP4, FMT_DPR, INFO_DPR = 1 << 0, 1 << 1, 1 << 2, 1 << 3, 1 << 4, 1 << 5
FMT_AD, FMT_ADF, FMT_ADR, INFO_AD, INFO_ADF, INFO_ADR = 1 << 6, 1 << 7, 1 << 8, 1 << 9, 1 << 10, 1 << 11
INFO_SCR, FMT_SCR, INFO_VDB, INFO_RPB, FMT_QS = 1 << 12, 1 << 13, 1 << 14, 1 << 15, 1 << 16
# CALL_* (call.h:32-39)
CALL_KEEPALT, CALL_VARONLY, CALL_FMT_PV4, CALL_FMT_GQ, CALL_FMT_GP = 1, 1 << 1, 1 << 5, 1 << 6, 1 << 7

MAX_ALLELES, MAX_PL, NPOS, NQUAL, MAX_DEPTH = 5, 15, 100, 60, 255
INT32_MISSING = -2147483648
INT32_VECTOR_END = -2147483647
GT_MISSING, GT_VECTOR_END = -1, -2

# FORMAT keys of an mpileup record in bcf_call2bcf's order (BCFGPU_BCF_*), each with the fmt_flag bit that selects it (PL: always)
BCF_KEYS = ("PL", "DP", "DV", "SP", "DP4", "ADF", "ADR", "AD", "DPR", "SCR", "QS")
BCF_KEY_FLAG = (0, FMT_DP, FMT_DV, FMT_SP, FMT_DP4, FMT_ADF, FMT_ADR, FMT_AD, FMT_DPR, FMT_SCR, FMT_QS)
# FORMAT keys of a call record that bcfgpu_call_encode_bcf writes (BCFGPU_CALL_BCF_*), each with an offset of its own per site
CALL_BCF_KEYS = ("GT", "PL", "GQ")
CALL_BCF_GT, CALL_BCF_PL, CALL_BCF_GQ, CALL_BCF_NKEYS = 0, 1, 2, 3

RD_REV, RD_SCLIP, RD_DEL, RD_SKIP = 1 << 20, 1 << 21, 1 << 22, 1 << 23


class Cfg(C.Structure):
    _fields_ = [
        ("device", C.c_int32), ("n_smpl", C.c_int32), ("max_sites", C.c_int32),
        ("max_reads", C.c_uint64),
        ("min_baseQ", C.c_int32), ("capQ", C.c_int32), ("errmod_theta", C.c_double),
        ("fmt_flag", C.c_int32),
        ("call_theta", C.c_double), ("call_flag", C.c_int32), ("output_tags", C.c_int32),
        ("n_grp", C.c_int32), ("grp_tag_is_qs", C.c_int32), ("ploidy_max", C.c_int32),
    ]


class Tile(C.Structure):
    _fields_ = [
        ("n_sites", C.c_int32), ("is_indel", C.c_int32), ("n_reads", C.c_uint64),
        ("ref16", C.c_void_p), ("plp_off", C.c_void_p), ("rd", C.c_void_p),
        ("epos", C.c_void_p), ("aux", C.c_void_p),
    ]


class Site(C.Structure):
    _fields_ = [
        ("a", C.c_int32 * 5), ("n_alleles", C.c_int32), ("unseen", C.c_int32),
        ("ori_ref", C.c_int32), ("shift", C.c_int32), ("ret", C.c_int32),
        ("depth", C.c_uint32), ("ori_depth", C.c_uint32), ("mq0", C.c_uint32),
        ("qsum", C.c_float * 5),
        ("vdb", C.c_float), ("mwu_pos", C.c_float), ("mwu_mq", C.c_float),
        ("mwu_bq", C.c_float), ("mwu_mqs", C.c_float), ("seg_bias", C.c_float),
        ("adf_tot", C.c_int32 * 5), ("adr_tot", C.c_int32 * 5),
        ("scr_tot", C.c_int32), ("pad", C.c_int32),
        ("anno", C.c_double * 16),
    ]


class MplpOut(C.Structure):
    _fields_ = [
        ("site", C.c_void_p), ("pl", C.c_void_p), ("dp4", C.c_void_p),
        ("adf", C.c_void_p), ("adr", C.c_void_p), ("qs", C.c_void_p), ("scr", C.c_void_p), ("sp", C.c_void_p),
    ]


class CallIn(C.Structure):
    _fields_ = [
        ("n_sites", C.c_int32), ("n_gt_max", C.c_int32), ("n_al_max", C.c_int32), ("reserved", C.c_int32),
        ("nals", C.c_void_p), ("unseen", C.c_void_p), ("pl", C.c_void_p), ("qs", C.c_void_p),
        ("ad", C.c_void_p), ("ploidy", C.c_void_p), ("grp", C.c_void_p),
        ("prior_an", C.c_void_p), ("prior_ac", C.c_void_p), ("i16", C.c_void_p),
    ]


class CallSite(C.Structure):
    _fields_ = [
        ("ret", C.c_int32), ("nals_new", C.c_int32), ("als_new", C.c_int32),
        ("als_map", C.c_int32 * 5), ("ac", C.c_int32 * 5), ("an", C.c_int32),
        ("qual_missing", C.c_int32), ("qual", C.c_float), ("pl_dropped", C.c_int32),
        ("has_i16", C.c_int32), ("dp4", C.c_int32 * 4), ("mq", C.c_int32), ("pv4_tested", C.c_int32), ("pv4", C.c_float * 4),
    ]


class CallOut(C.Structure):
    _fields_ = [
        ("site", C.c_void_p), ("gt", C.c_void_p), ("pl", C.c_void_p),
        ("gq", C.c_void_p), ("gp", C.c_void_p),
    ]


class Reads(C.Structure):
    _fields_ = [("n_reads", C.c_int32)] + [(k, C.c_void_p) for k in
                ("r_pos", "r_lq", "r_flag", "r_ncig", "r_cig_off", "r_seq_off", "cig", "seq16", "qual", "zq", "r_has_zq")]


class Packed(C.Structure):
    """bcfgpu_packed: the pool as BAM records hold it (4-bit bases, optional 4-bit palette qualities)."""
    _fields_ = [("seq4", C.c_void_p), ("qual4", C.c_void_p), ("palette", C.c_uint8 * 16), ("n_bases", C.c_int64), ("n_cig", C.c_int64),
                ("smpl_off", C.c_void_p), ("qual_bits", C.c_int32), ("recs", C.c_void_p)]


def pack_nibbles(a):
    """Two 4-bit values per byte, the even index in the high nibble (bam_get_seq's order); odd lengths padded with 0."""
    import numpy as np
    a = np.asarray(a, np.uint8)
    if a.size & 1:
        a = np.concatenate([a, np.zeros(1, np.uint8)])
    return ((a[0::2] << 4) | (a[1::2] & 15)).astype(np.uint8)


READ12 = [("pos", "<i4"), ("lq", "<u2"), ("ncig", "u1"), ("flag8", "u1"), ("mapq", "u1"), ("pad", "u1", 3)]     # bcfgpu_read12


def read12(r_pos, r_lq, r_ncig, r_flag, r_mapq):
    """The per-read arrays as bcfgpu_read12 records (numpy structured array, 12 bytes a read)."""
    import numpy as np
    rec = np.zeros(len(r_pos), dtype=READ12)
    rec["pos"], rec["lq"], rec["ncig"], rec["mapq"] = r_pos, r_lq, r_ncig, r_mapq
    rec["flag8"] = ((np.asarray(r_flag) & 16) != 0) * 1 + ((np.asarray(r_flag) & 4) != 0) * 2
    return rec


def pack_crumbs(a):
    """Four 2-bit values per byte, index 0 in the two highest bits; lengths padded to a multiple of four with 0."""
    import numpy as np
    a = np.asarray(a, np.uint8)
    if a.size & 3:
        a = np.concatenate([a, np.zeros(4 - (a.size & 3), np.uint8)])
    return ((a[0::4] << 6) | ((a[1::4] & 3) << 4) | ((a[2::4] & 3) << 2) | (a[3::4] & 3)).astype(np.uint8)


class IndelIn(C.Structure):
    _fields_ = [("n_sites", C.c_int32), ("n_smpl", C.c_int32), ("pos", C.c_void_p), ("smpl_off", C.c_void_p),
                ("p_read", C.c_void_p), ("p_qpos", C.c_void_p), ("p_indel", C.c_void_p), ("ref", C.c_char_p),
                ("openQ", C.c_int32), ("extQ", C.c_int32), ("tandemQ", C.c_int32), ("min_support", C.c_int32),
                ("per_sample_flt", C.c_int32), ("min_frac", C.c_double)]


class IndelOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("ret", "p_aux", "indel_types", "inscns", "maxins", "indelreg", "max_support", "max_frac")]


class GvcfBlock(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("first_site", "last_site", "start_pos", "end1", "min_dp", "range")]


class GvcfIn(C.Structure):
    _fields_ = [("n_sites", C.c_int32), ("n_range", C.c_int32)] + [(k, C.c_void_p) for k in
                ("dp_range", "pos", "rid", "brk", "site", "pl", "dp4", "ref_only", "dp", "end")]


class GvcfOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("blk", "min_dp", "block", "dp", "pl")]


class GapStats(C.Structure):
    _fields_ = [("n_jobs", C.c_uint64), ("n_passes", C.c_uint64), ("dp_cells", C.c_uint64),
                ("kernel_ms", C.c_float), ("prepare_ms", C.c_float), ("finalize_ms", C.c_float), ("total_ms", C.c_float),
                ("n_wide", C.c_uint64), ("n_scratch", C.c_uint64), ("band_jobs", C.c_uint32 * 8)]


class BcfVec(C.Structure):
    """bcfgpu_bcf_vec: where one FORMAT key's values of a BCF record lie in the per-sample bytes."""
    _fields_ = [("off", C.c_uint64), ("type", C.c_int32), ("width", C.c_int32)]


BCF_VEC = [("off", "<u8"), ("type", "<i4"), ("width", "<i4")]       # the same as a numpy record



class VcfVec(C.Structure):
    """bcfgpu_vcf_vec: where a VCF record's sample columns lie in the text buffer, and the key's place in its FORMAT column."""
    _fields_ = [("off", C.c_uint64), ("len", C.c_uint32), ("idx", C.c_int32)]


VCF_VEC = [("off", "<u8"), ("len", "<u4"), ("idx", "<i4")]
VCFDEC_START_BYTES = 4 << 20        # BCFGPU_VCFDEC_START_BYTES: the bound on the workspace of bcfgpu_call_decode_vcf's column offsets

# bcfgpu_call_constrain: the modes (BCFGPU_CALS_NUMBER_*) and the bound on n_in / n_out
CALS_NUMBER_G, CALS_NUMBER_R = 0, 1
CALS_MAX_PLANES = 1 << 20


class CalsSite(C.Structure):
    """bcfgpu_cals_site: one record of bcfgpu_call_constrain -- the alleles of the constrained record, the unseen allele before the
    rewrite, whether the record changes, new allele -> original allele (32 bytes)."""
    _fields_ = [("n_new", C.c_int32), ("unseen", C.c_int32), ("changed", C.c_int32), ("amap", C.c_int32 * 5)]


CALS_SITE = [("n_new", "<i4"), ("unseen", "<i4"), ("changed", "<i4"), ("amap", "<i4", (5,))]

BCF_KEY_MAX_WIDTH = 255


class BcfKey(C.Structure):
    """bcfgpu_bcf_key: one pass-through FORMAT key of one record, a job of bcfgpu_call_remap_bcf (32 bytes)."""
    _fields_ = [("off", C.c_uint64), ("site", C.c_int32), ("key_id", C.c_int32), ("type", C.c_int32), ("width", C.c_int32),
                ("nals", C.c_int32), ("flags", C.c_int32)]


BCF_KEY = [("off", "<u8"), ("site", "<i4"), ("key_id", "<i4"), ("type", "<i4"), ("width", "<i4"), ("nals", "<i4"), ("flags", "<i4")]


# bcfgpu_call_encode_vcf: the kinds of a field (BCFGPU_VCF_FIELD_*), the fields a site may have, the bound on one sample's text
VCF_FIELD_GT, VCF_FIELD_PL, VCF_FIELD_GQ, VCF_FIELD_KEY = 0, 1, 2, 3
VCF_MAX_FIELDS = 16
VCF_SAMPLE_CAP = 15360


class VcfField(C.Structure):
    """bcfgpu_vcf_field: one field of one record's sample column, for bcfgpu_call_encode_vcf (32 bytes, the layout of BcfKey)."""
    _fields_ = [("off", C.c_uint64), ("site", C.c_int32), ("kind", C.c_int32), ("type", C.c_int32), ("width", C.c_int32),
                ("nals", C.c_int32), ("flags", C.c_int32)]


VCF_FIELD = [("off", "<u8"), ("site", "<i4"), ("kind", "<i4"), ("type", "<i4"), ("width", "<i4"), ("nals", "<i4"), ("flags", "<i4")]


# bcfgpu_call_rewrite_vcf: the most FORMAT keys of a record (a bit of r_mask each)
VCF_REWRITE_MAX_KEYS = 64


class VcfRewrite(C.Structure):
    """bcfgpu_vcf_rewrite: one record of bcfgpu_call_rewrite_vcf -- where its sample columns lie in the text buffer, which of its
    FORMAT keys are Number=R, PL's place, the keys' and alleles' counts, whether PL and GQ are listed (32 bytes)."""
    _fields_ = [("off", C.c_uint64), ("r_mask", C.c_uint64), ("len", C.c_uint32), ("pl_idx", C.c_int32), ("n_fmt", C.c_int16),
                ("nals", C.c_int16), ("flags", C.c_int32)]


VCF_REWRITE = [("off", "<u8"), ("r_mask", "<u8"), ("len", "<u4"), ("pl_idx", "<i4"), ("n_fmt", "<i2"), ("nals", "<i2"), ("flags", "<i4")]


class VcfKey(C.Structure):
    """bcfgpu_vcf_key: one integer pass-through FORMAT key of one record of VCF text input, a job of bcfgpu_call_parse_keys_vcf (32 bytes)."""
    _fields_ = [("site", C.c_int32), ("key_id", C.c_int32), ("idx", C.c_int32), ("nals", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 3)]


VCF_KEY = [("site", "<i4"), ("key_id", "<i4"), ("idx", "<i4"), ("nals", "<i4"), ("flags", "<i4"), ("reserved", "<i4", (3,))]


class Timing(C.Structure):
    _fields_ = [("glfgen_ms", C.c_float), ("combine_ms", C.c_float),
                ("mcall_ms", C.c_float), ("total_ms", C.c_float)]


# every symbol include/bcfgpu.h declares: name -> (restype, argtypes)
PROTOTYPES = {
    "bcfgpu_create": (C.c_int, [C.POINTER(Cfg), C.POINTER(C.c_void_p)]),
    "bcfgpu_destroy": (None, [C.c_void_p]),
    "bcfgpu_last_error": (C.c_char_p, []),
    "bcfgpu_device_count": (C.c_int, []),
    "bcfgpu_malloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "bcfgpu_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bcfgpu_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "bcfgpu_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "bcfgpu_memset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t]),
    "bcfgpu_sync": (C.c_int, [C.c_void_p]),
    "bcfgpu_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "bcfgpu_host_free": (C.c_int, [C.c_void_p]),
    "bcfgpu_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bcfgpu_pack_read": (None, [C.c_int] * 9 + [C.c_void_p, C.c_int, C.c_int,
                                                C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]),
    "bcfgpu_mpileup": (C.c_int, [C.c_void_p, C.POINTER(Tile), C.POINTER(MplpOut)]),
    "bcfgpu_mcall": (C.c_int, [C.c_void_p, C.POINTER(CallIn), C.POINTER(CallOut)]),
    "bcfgpu_gap_prep": (C.c_int, [C.c_void_p, C.POINTER(Reads), C.POINTER(IndelIn), C.POINTER(IndelOut), C.c_int]),
    "bcfgpu_gap_prep_tile": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(Reads), C.POINTER(IndelIn), C.POINTER(IndelOut), C.c_int,
                                       C.POINTER(Tile)]),
    "bcfgpu_baq": (C.c_int, [C.c_void_p, C.POINTER(Reads), C.c_char_p, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcfgpu_cap_mapq": (C.c_int, [C.c_void_p, C.POINTER(Reads), C.c_char_p, C.c_int32, C.c_int32, C.c_void_p]),
    "bcfgpu_overlap_tweak": (C.c_int, [C.c_void_p, C.POINTER(Reads), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcfgpu_pileup_indel_tile": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(Tile)]),
    "bcfgpu_pileup_entries": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "bcfgpu_pileup": (C.c_int, [C.c_void_p, C.POINTER(Reads), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_int32,
                                C.POINTER(Tile), C.c_void_p, C.c_void_p]),
    "bcfgpu_pileup_packed": (C.c_int, [C.c_void_p, C.POINTER(Reads), C.POINTER(Packed), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_char_p,
                                       C.c_int32, C.POINTER(Tile), C.c_void_p, C.c_void_p]),
    "bcfgpu_pool_upload": (C.c_int, [C.c_void_p, C.POINTER(Reads), C.POINTER(Packed), C.c_void_p]),
    "bcfgpu_pool_stage": (C.c_int, [C.c_void_p, C.POINTER(Reads), C.POINTER(Packed), C.c_void_p]),
    "bcfgpu_pool_adopt": (C.c_int, [C.c_void_p]),
    "bcfgpu_pool_baq": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_int, C.c_void_p]),
    "bcfgpu_pool_cap_mapq": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_void_p]),
    "bcfgpu_pool_keep": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bcfgpu_pool_overlap_tweak": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "bcfgpu_pool_pileup": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(Tile),
                                     C.c_void_p, C.c_void_p]),
    "bcfgpu_pool_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bcfgpu_gvcf_blocks": (C.c_int, [C.c_void_p, C.POINTER(GvcfIn), C.POINTER(GvcfOut), C.POINTER(C.c_int32)]),
    "bcfgpu_gap_prep_stats": (C.c_int, [C.c_void_p, C.POINTER(GapStats)]),
    "bcfgpu_pipeline": (C.c_int, [C.c_void_p, C.POINTER(Tile), C.c_void_p, C.c_void_p,
                                  C.POINTER(MplpOut), C.POINTER(CallOut)]),
    "bcfgpu_mplp_out_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "bcfgpu_truncated_cells": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "bcfgpu_errmod_plan": (C.c_int, [C.c_void_p, C.POINTER(Tile), C.POINTER(Tile), C.c_void_p, C.c_void_p]),
    "bcfgpu_errmod_plan_visit": (C.c_int, [C.c_void_p, C.POINTER(Tile), C.c_void_p, C.POINTER(Tile), C.c_void_p, C.c_void_p]),
    "bcfgpu_errmod_seed": (C.c_int, [C.c_void_p, C.c_uint64]),
    "bcfgpu_errmod_state": (C.c_uint64, [C.c_void_p]),
    "bcfgpu_depth_cap": (C.c_int, [C.POINTER(Reads), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "bcfgpu_depth_cap_new": (C.c_void_p, [C.c_int32, C.c_int32]),
    "bcfgpu_depth_cap_push": (C.c_int, [C.c_void_p, C.POINTER(Reads), C.c_void_p, C.c_void_p]),
    "bcfgpu_depth_cap_reset": (None, [C.c_void_p]),
    "bcfgpu_depth_cap_free": (None, [C.c_void_p]),
    "bcfgpu_compact_calls": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(CallOut), C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "bcfgpu_compact_calls_async": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(CallOut), C.c_int32, C.c_int32, C.c_void_p,
                                             C.c_uint64, C.c_void_p]),
    "bcfgpu_compact_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "bcfgpu_mplp_encode_bcf": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MplpOut), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_uint64,
                                         C.c_void_p, C.POINTER(C.c_uint64)]),
    "bcfgpu_mplp_encode_vcf": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MplpOut), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                         C.POINTER(C.c_uint64)]),
    "bcfgpu_call_encode_bcf": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(CallOut), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p,
                                         C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "bcfgpu_call_decode_bcf": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(BcfVec), C.POINTER(C.c_int32),
                                         C.c_int32, C.c_void_p]),
    "bcfgpu_call_decode_vcf": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(VcfVec), C.POINTER(C.c_int32),
                                         C.c_int32, C.c_void_p]),
    "bcfgpu_call_constrain": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(CalsSite), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "bcfgpu_call_remap_bcf": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(BcfKey), C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_int32),
                                        C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "bcfgpu_call_encode_vcf": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(CallOut), C.c_int32, C.POINTER(VcfField), C.c_int32, C.c_void_p,
                                         C.c_uint64, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "bcfgpu_call_rewrite_vcf": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(CallOut), C.POINTER(VcfRewrite), C.c_int32, C.c_void_p,
                                          C.c_uint64, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "bcfgpu_call_parse_keys_vcf": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(VcfKey), C.c_int32, C.POINTER(VcfVec), C.c_int32, C.c_void_p, C.c_uint64,
                                             C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64),
                                             C.c_void_p]),
    "bcfgpu_comm_init_all":(C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p)]),
    "bcfgpu_comm_destroy": (None, [C.c_void_p]),
    "bcfgpu_gather_bytes": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    "bcfgpu_timing_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "bcfgpu_timing_get": (C.c_int, [C.c_void_p, C.POINTER(Timing)]),
    "bcfgpu_abi_sizes": (None, [C.POINTER(C.c_int32)]),
}


def default_cfg(n_smpl, max_sites=0, max_reads=0, device=0, fmt_flag=INFO_VDB | INFO_RPB,
                min_baseQ=13, call_theta=1.1e-3, call_flag=0, output_tags=0, n_grp=1):
    """Defaults of `bcftools mpileup` (mpileup.c:937-950) and `bcftools call -m` (vcfcall.c:931-943)."""
    c = Cfg()
    c.device, c.n_smpl, c.max_sites, c.max_reads = device, n_smpl, max_sites, max_reads
    c.min_baseQ, c.capQ, c.errmod_theta, c.fmt_flag = min_baseQ, 60, 0.0, fmt_flag
    c.call_theta, c.call_flag, c.output_tags = call_theta, call_flag, output_tags
    c.n_grp, c.grp_tag_is_qs, c.ploidy_max = n_grp, 0, 2
    return c
