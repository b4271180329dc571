"""What bcfgpu_call_parse_keys_vcf is to produce, on Python strings and ints: the integer pass-through FORMAT keys of a call record
of VCF text input (AD, ADF, ADR, DP, SP, ...) as BCF2 key blocks, from the input record's own sample columns.  The rule is the text
route's -- the columns split and printed again by host/bcfgpu_call.c, then parsed and narrowed by host/vcfio.c -- stated on the text:

    token    a called sample reads input column col[s] (or s); the column is cut at ':' and token idx is the key's text; a column
             with fewer tokens (a whole-column '.' included) has the token '.'
    values   the token is cut at ',': '.' is `missing`, [+-]?[0-9]+ inside int32 its value (leading zeros allowed; the decimal text
             of the two int32 sentinels is stored as it stands)
    remap    Number=R and alleles dropped (nals_new != nals) and the token present with exactly nals values: [v[0]] when one allele is
             left, else nals_new values `missing` with out[als_map[i]] = v[i] for the kept alleles; every other vector as it is
    width    the longest output vector over the called samples, shorter ones padded with `end of vector`
    type     the smallest of int8 / int16 / int32 that holds every output value which is no sentinel
    status   1 when any value of token idx of a called sample's column is neither '.' nor [+-]?[0-9]+ inside int32 (an empty value
             counts; every value is checked, kept by the remap or not); 2 when the width passes 255; a flagged job has no block

Written from the entry's statement in include/bcfgpu.h and the BCF2 specification, not from the kernel; the block layout is
tests/helpers/callenc.encode_vectors.  Test infrastructure: the yardstick for bcfgpu_call_parse_keys_vcf (pinned against the host
writer and the reference's goldens in tests/test_call_key_text_encoder.py)."""
import re

import numpy as np

from tests.helpers.callenc import MISSING, VEND, encode_vectors

MAX_ALLELES = 5
MAX_WIDTH = 255                                                 # BCFGPU_BCF_KEY_MAX_WIDTH
MAX_KEYS = 64                                                   # BCFGPU_VCF_REWRITE_MAX_KEYS
# bcfgpu_vcf_key / bcfgpu_vcf_vec as numpy records (bcftools_amd.abi.VCF_KEY / VCF_VEC, restated: the twin stands alone)
KEY_DTYPE = np.dtype([("site", "<i4"), ("key_id", "<i4"), ("idx", "<i4"), ("nals", "<i4"), ("flags", "<i4"), ("reserved", "<i4", (3,))])
RUN_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("idx", "<i4")])
_INT = re.compile(r"[+-]?[0-9]+\Z")


def parse_token(token):
    """The token's values and whether every one of them is '.' or an integer inside int32: (values, ok).  A value that is not has
    None in its place."""
    vals, ok = [], True
    for t in token.split(","):
        if t == ".":
            vals.append(MISSING)
        elif _INT.match(t) and -2147483648 <= int(t) <= 2147483647:
            vals.append(int(t))
        else:
            vals.append(None)
            ok = False
    return vals, ok


def column_token(column, idx):
    """(token idx of the column's text, whether the column has it)."""
    toks = column.split(":")
    return (toks[idx], True) if idx < len(toks) else (".", False)


def output_vector(values, present, nals, flags, nn, als_map):
    """The vector a sample's values become."""
    if (flags & 1) and nn != nals and present and len(values) == nals:
        if nn == 1:
            return [values[0]]
        out = [MISSING] * nn
        for i in range(nals):
            if als_map[i] >= 0:
                out[als_map[i]] = values[i]
        return out
    return list(values)


def encode_key(key_id, columns, idx, nals=1, flags=0, nn=None, als_map=None, col=None):
    """One job: columns = the input samples' column texts (without their tabs).  Returns (block, status)."""
    nn = nals if nn is None else max(1, min(MAX_ALLELES, int(nn)))
    als_map = list(range(MAX_ALLELES)) if als_map is None else [int(x) for x in als_map]
    vecs, ok = [], True
    for c in (range(len(columns)) if col is None else col):
        token, present = column_token(columns[c], idx)
        values, good = parse_token(token)
        ok &= good
        if good:
            vecs.append(output_vector(values, present, nals, flags, nn, als_map))
    if not ok:
        return b"", 1
    if max(len(v) for v in vecs) > MAX_WIDTH:
        return b"", 2
    return encode_vectors(key_id, vecs), 0


def split_run(text, run, n_smpl_in):
    """The n_smpl_in column texts of a run: a tab in front of each."""
    raw = bytes(text[int(run["off"]):int(run["off"]) + int(run["len"])]).decode("latin-1")
    assert raw[:1] == "\t" and raw.count("\t") == n_smpl_in
    return raw[1:].split("\t")


def encode_jobs(text, run, keys, n_smpl_in, site, n_smpl, col=None, emit=None):
    """text: the records' sample columns (bytes); run: records of RUN_DTYPE, one a site; keys: records of KEY_DTYPE; site: per site
    nals_new and als_map.  Returns (np.uint8 bytes, np.uint64 offsets [n_keys + 1], np.uint8 status [n_keys])."""
    assert col is not None or n_smpl <= n_smpl_in
    use = list(range(n_smpl)) if col is None else [int(c) for c in col]
    assert len(use) == n_smpl
    data, off, status = bytearray(), [0], []
    for k in keys:
        s, st = int(k["site"]), 0
        if emit is None or emit[s]:
            block, st = encode_key(int(k["key_id"]), split_run(text, run[s], n_smpl_in), int(k["idx"]), int(k["nals"]), int(k["flags"]),
                                   site[s]["nals_new"], site[s]["als_map"], use)
            data += block
        status.append(st)
        off.append(len(data))
    return np.frombuffer(bytes(data), np.uint8), np.array(off, np.uint64), np.array(status, np.uint8)
