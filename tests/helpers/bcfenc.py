"""The per-sample ("indiv") part of a BCF2 record for integer FORMAT fields, in numpy, from the rules of the BCF2
specification (VCFv4.2 / BCFv2.2, section 6.3.3 "Type encoding" and 6.3.2 "Genotype fields"):

  * a typed value starts with a descriptor byte: the number of elements in the high four bits, the type in the low four
    (1 = int8, 2 = int16, 3 = int32); 15 in the high bits means "the count follows as a typed integer";
  * an integer is stored little-endian in the smallest type that holds it; a vector in the smallest type that holds all of
    its values;
  * per FORMAT field: the key's dictionary index as a typed integer, then one descriptor (elements per sample, type) for
    all samples, then the samples' vectors back to back.

Values here are non-negative and carry no missing / end-of-vector sentinel (an mpileup record has none), so the type
bounds are the plain ones: 127 and 32767.  Test infrastructure: the yardstick for bcfgpu_mplp_encode_bcf.
"""
import numpy as np

from bcftools_amd import abi

KEYS = abi.BCF_KEYS
_DTYPE = {1: "<i1", 2: "<i2", 3: "<i4"}


def int_type(mx):
    return 1 if mx <= 127 else 2 if mx <= 32767 else 3


def typed_int(x):
    """One integer as a typed value: descriptor (one element) and the value."""
    t = int_type(x)
    return bytes([0x10 | t]) + np.array([x], _DTYPE[t]).tobytes()


def descriptor(width, t):
    if width < 15:
        return bytes([width << 4 | t])
    return bytes([0xF0 | t]) + typed_int(width)


def encode_key(key_id, vals):
    """vals: [n_smpl][width] non-negative integers -> the field's bytes."""
    vals = np.asarray(vals, dtype=np.int64)
    assert vals.ndim == 2 and vals.size and vals.min() >= 0
    t = int_type(int(vals.max()))
    return typed_int(key_id) + descriptor(vals.shape[1], t) + np.ascontiguousarray(vals.astype(_DTYPE[t])).tobytes()


def encode_fields(fields):
    """fields: [(key id, vals [n_smpl][width])] in record order -> the indiv block."""
    return b"".join(encode_key(i, v) for i, v in fields)


def key_values(key, na, pl, dp4, adf, adr, qs, scr, sp):
    """[n_smpl][width] of one key at one site from that site's planes ([plane][n_smpl]; None where not given)."""
    i64 = lambda a: np.asarray(a, np.int64)
    if key == "PL":
        return i64(pl[:na * (na + 1) // 2]).T
    if key == "DP":
        return i64(dp4).sum(0)[:, None]
    if key == "DV":
        return i64(dp4[2:4]).sum(0)[:, None]
    if key == "SP":
        return i64(sp)[:, None]
    if key == "DP4":
        return i64(dp4).T
    if key == "ADF":
        return i64(adf[:na]).T
    if key == "ADR":
        return i64(adr[:na]).T
    if key in ("AD", "DPR"):
        return (i64(adf[:na]) + i64(adr[:na])).T
    if key == "SCR":
        return i64(scr)[:, None]
    if key == "QS":
        return i64(qs[:na]).T
    raise KeyError(key)


def selected_keys(fmt_flag):
    return [k for k, f in zip(KEYS, abi.BCF_KEY_FLAG) if k == "PL" or fmt_flag & f]


def encode_planes(fmt_flag, key_id, n_alleles, pl, dp4, adf=None, adr=None, qs=None, scr=None, sp=None, emit=None):
    """What bcfgpu_mplp_encode_bcf is to produce from the planes of a tile ([site][plane][n_smpl], as bcfgpu_mplp_out):
    (bytes, offsets [n_sites + 1]).  key_id: {name: dictionary index}."""
    n = len(n_alleles)
    keys = selected_keys(fmt_flag)
    out, off = [], np.zeros(n + 1, np.uint64)
    at = 0
    for k in range(n):
        if emit is None or emit[k]:
            g = lambda a: None if a is None else a[k]
            b = encode_fields([(key_id[key], key_values(key, int(n_alleles[k]), pl[k], dp4[k], g(adf), g(adr), g(qs), g(scr), g(sp)))
                               for key in keys])
            out.append(b)
            at += len(b)
        off[k + 1] = at
    return np.frombuffer(b"".join(out), np.uint8), off
