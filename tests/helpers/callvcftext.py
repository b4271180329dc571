"""What bcfgpu_call_rewrite_vcf is to produce, in Python: the sample columns of a call record of VCF text input, rewritten from the
input record's own columns around the caller's GT, PL and GQ planes.  The rule is the text route's -- host/bcfgpu_call.c
print_sample_text / print_gt / print_numberR over the input column's text -- stated with string splits:

    a sample   a tab, then its fields joined by ':'; no newline.  Called sample s reads input column col[s] (s without a map)
    GT         first (tests/helpers/callvcf.py gt_text)
    keys       the input column split at ':' into nv tokens; for key i < n_fmt: at PL's place the PL text (callvcf.pl_text) when the
               record lists PL, nothing -- no ':' either -- when it does not; elsewhere token i, '.' when i >= nv.  A token of a
               Number=R key of a record that lost alleles is split at ',': with exactly nals values it becomes value 0 when nn == 1,
               else nn values '.' with out[map[j]] = value[j] for every j < nals with map[j] >= 0; any other token stays as it is
    GQ         last, when the record lists it

Written from the rule, not from the kernel.  Test infrastructure: the yardstick for bcfgpu_call_rewrite_vcf (pinned against the
reference's `call` goldens in tests/test_call_rewrite_text.py)."""
import numpy as np

from tests.helpers.callvcf import MAX_ALLELES, gt_text, pl_text, value_text

MAX_KEYS = 64
FLAG_PL, FLAG_GQ = 1, 2
# bcfgpu_vcf_rewrite as a numpy record (bcftools_amd.abi.VCF_REWRITE, restated: the twin stands alone)
REC_DTYPE = [("off", "<u8"), ("r_mask", "<u8"), ("len", "<u4"), ("pl_idx", "<i4"), ("n_fmt", "<i2"), ("nals", "<i2"), ("flags", "<i4")]


def number_r(token, nals, nn, als_map):
    """print_numberR: a Number=R token of a record whose alleles went from nals to nn != nals."""
    v = token.split(b",")
    if len(v) != nals:
        return token
    if nn == 1:
        return v[0]
    out = [b"."] * nn
    for j in range(nals):
        if 0 <= als_map[j] < nn:
            out[als_map[j]] = v[j]
    return b",".join(out)


def sample_text(column, rec, nn, als_map, gt, pl, gq, ngn):
    """column: the input column's bytes without its tab; gt: (g0, g1); pl: the sample's values of the PL planes or None; gq: its
    value or None.  The sample's text, tab included."""
    tokens = column.split(b":")
    n_fmt, pl_idx, nals, flags, r_mask = int(rec["n_fmt"]), int(rec["pl_idx"]), int(rec["nals"]), int(rec["flags"]), int(rec["r_mask"])
    out = [gt_text(*gt).encode()]
    for i in range(n_fmt):
        if i == pl_idx:
            if flags & FLAG_PL:
                out.append(pl_text(pl, ngn).encode())
            continue
        if i >= len(tokens):
            out.append(b".")
        elif (r_mask >> i) & 1 and nn != nals:
            out.append(number_r(tokens[i], nals, nn, als_map))
        else:
            out.append(tokens[i])
    if flags & FLAG_GQ:
        out.append(value_text(gq).encode())
    return b"\t" + b":".join(out)


def columns_of(text, rec, n_smpl_in):
    """The n_smpl_in input columns of the record's run, without their tabs."""
    run = bytes(text[int(rec["off"]):int(rec["off"]) + int(rec["len"])])
    assert run[:1] == b"\t"
    cols = run[1:].split(b"\t")
    assert len(cols) == n_smpl_in
    return cols


def site_texts(planes, n_gt_max, rec, text, n_smpl_in, site, n_smpl, col=None):
    """One site (planes: this site's gt [2][S], pl [n_gt_max][S], gq [S], absent ones None): per called sample the text."""
    nn = min(max(int(site["nals_new"]), 1), MAX_ALLELES)
    ngn = min(nn * (nn + 1) // 2, n_gt_max)
    als_map = [int(x) for x in site["als_map"]]
    cols = columns_of(text, rec, n_smpl_in)
    pick = list(col) if col is not None else list(range(n_smpl))
    out = []
    for s in range(n_smpl):
        pl = planes["pl"][:, s] if planes.get("pl") is not None else None
        gq = int(planes["gq"][s]) if planes.get("gq") is not None else None
        out.append(sample_text(cols[pick[s]], rec, nn, als_map, (int(planes["gt"][0][s]), int(planes["gt"][1][s])), pl, gq, ngn))
    return out


def rewrite(planes, n_gt_max, rec, text, n_smpl_in, site, n_smpl, col=None, emit=None):
    """planes: {"gt": [n][2][S], "pl": [n][n_gt_max][S], "gq": [n][S]} (pl / gq may be absent when no record lists them); rec: records
    of REC_DTYPE, one a site; text: the byte buffer; site: records with nals_new and als_map.  Returns (np.uint8 bytes, np.uint64
    offsets [n_sites + 1])."""
    text = bytes(text)
    data, off = bytearray(), [0]
    for k in range(len(rec)):
        if emit is None or emit[k]:
            here = {name: planes[name][k] for name in ("gt", "pl", "gq") if planes.get(name) is not None}
            data += b"".join(site_texts(here, n_gt_max, rec[k], text, n_smpl_in, site[k], n_smpl, col))
        off.append(len(data))
    return np.frombuffer(bytes(data), np.uint8), np.array(off, np.uint64)
