"""What bcfgpu_call_encode_vcf is to produce, in Python / numpy: the sample columns of a call record as VCF text, the caller's GT, PL
and GQ planes and the pass-through keys of the input record's bytes interleaved in the order of the record's FORMAT column.  The
rule is the text route's -- host/bcfgpu_call.c print_sample_text / print_gt / print_numberR over host/vcfio.c vio_indiv_text --
stated on the values:

    a sample   a tab, then its site's fields joined by ':'; no newline
    GT         the first entry as its digit, '.' when missing; '/' and the second entry unless that is `end of vector`
    PL         planes 0 .. ngn-1 up to the first `end of vector`, joined by ',', '.' for missing; nothing printed: '.'
    GQ         one value, '.' for missing
    KEY        the vector and remap of tests/helpers/keyenc.py (sample_vector, remap), joined by ',', '.' for missing

Written from the rule, not from the kernel.  Test infrastructure: the yardstick for bcfgpu_call_encode_vcf (pinned against the
reference's `call` goldens in tests/test_call_sample_text.py)."""
import numpy as np

from tests.helpers import keyenc
from tests.helpers.callenc import GT_MISSING, GT_VEND, MISSING, VEND

GT, PL, GQ, KEY = 0, 1, 2, 3
MAX_FIELDS, SAMPLE_CAP, MAX_ALLELES = 16, 15360, 5
# bcfgpu_vcf_field as a numpy record (bcftools_amd.abi.VCF_FIELD, restated: the twin stands alone)
FIELD_DTYPE = [("off", "<u8"), ("site", "<i4"), ("kind", "<i4"), ("type", "<i4"), ("width", "<i4"), ("nals", "<i4"), ("flags", "<i4")]


def value_text(v):
    return "." if v == MISSING else str(int(v))


def gt_text(g0, g1):
    def one(g):
        return str(int(g)) if 0 <= g <= 9 else "."
    return one(g0) if g1 == GT_VEND else one(g0) + "/" + one(g1)


def pl_text(column, ngn):
    """column: one sample's values of the PL planes."""
    out = []
    for j in range(ngn):
        v = int(column[j])
        if v == VEND:
            break
        out.append(value_text(v))
    return ",".join(out) or "."


def field_bound(f, n_gt_max):
    """values x (longest text of a value + 1): a field's share of the bound on one sample's text (include/bcfgpu.h)."""
    kind = int(f["kind"])
    if kind == GT:
        return 4
    if kind == PL:
        return n_gt_max * 12
    if kind == GQ:
        return 12
    t, w = int(f["type"]), int(f["width"])
    values = max(w if t else 0, 1)
    if int(f["flags"]) & 1:
        values = max(values, MAX_ALLELES)
    return values * {0: 5, 1: 5, 2: 7, 3: 12}[t]


def site_bound(fields, n_gt_max):
    """The bound on one sample's text of a site with these fields."""
    return 1 + sum(field_bound(f, n_gt_max) for f in fields)


def sample_texts(planes, n_gt_max, fields, indiv, n_smpl_in, site, n_smpl, col=None):
    """One site (fields: its fields in order; site: its record; planes: this site's gt [2][S], pl [n_gt_max][S], gq [S], absent
    ones None): per called sample the text, tab included."""
    nn = min(max(int(site["nals_new"]), 1), MAX_ALLELES)
    ngn = min(nn * (nn + 1) // 2, n_gt_max)
    cols = list(col) if col is not None else list(range(n_smpl))
    per_field = []
    for f in fields:
        kind = int(f["kind"])
        if kind == GT:
            per_field.append([gt_text(int(planes["gt"][0][s]), int(planes["gt"][1][s])) for s in range(n_smpl)])
        elif kind == PL:
            per_field.append([pl_text(planes["pl"][:, s], ngn) for s in range(n_smpl)])
        elif kind == GQ:
            per_field.append([value_text(int(planes["gq"][s])) for s in range(n_smpl)])
        else:
            assert kind == KEY
            vecs = keyenc.output_vectors(indiv[int(f["off"]):], int(f["type"]), int(f["width"]) if int(f["type"]) else 0, n_smpl_in, int(f["nals"]),
                                         int(f["flags"]), nn, [int(x) for x in site["als_map"]], cols)
            per_field.append([",".join(value_text(v) for v in vec) for vec in vecs])
    return ["\t" + ":".join(pf[s] for pf in per_field) for s in range(n_smpl)]


def encode_fields(planes, n_gt_max, fields, indiv, n_smpl_in, site, n_smpl, col=None, emit=None):
    """planes: {"gt": [n][2][S], "pl": [n][n_gt_max][S], "gq": [n][S]} (a plane no field reads may be absent); fields: records of
    FIELD_DTYPE, ordered by site; indiv: the byte buffer; site: records with nals_new and als_map.  Returns (np.uint8 bytes,
    np.uint64 offsets [n_sites + 1])."""
    indiv = bytes(indiv)
    by_site = {}
    for f in fields:
        by_site.setdefault(int(f["site"]), []).append(f)
    data, off = bytearray(), [0]
    for k in range(len(site)):
        fs = by_site.get(k, [])
        if fs and (emit is None or emit[k]):
            here = {name: planes[name][k] for name in ("gt", "pl", "gq") if planes.get(name) is not None}
            data += "".join(sample_texts(here, n_gt_max, fs, indiv, n_smpl_in, site[k], n_smpl, col)).encode()
        off.append(len(data))
    return np.frombuffer(bytes(data), np.uint8), np.array(off, np.uint64)
