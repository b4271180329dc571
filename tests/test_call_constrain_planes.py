"""The numpy twin of tests/helpers/calsplanes.py -- the yardstick bcfgpu_call_constrain is compared with -- pinned against the record
rewrite of tests/helpers/cals.py (constrain_record, itself pinned to the reference's nine `-C alleles` goldens through the call tests):
on every record that the nine inputs pair with a target, the planes parsed from the constrained record's text (PL, and AD where the
file has it) equal the twin applied to the planes parsed from the original record's text, with the descriptor the head of the record
and its target give.  CPU only."""
import os

import numpy as np
import pytest

from tests.helpers import cals, calsplanes as CP, vcf as V

CALS_ROWS = [
    ("mpileup.vcf", "mpileup.tab", False), ("mpileup.2.vcf", "mpileup.2.tab", False),
    ("mpileup.3.vcf", "mpileup.3.tab", True), ("mpileup.3.vcf", "mpileup.4.tab", True),
    ("mpileup.3.vcf", "mpileup.5.tab", True), ("mpileup.4.vcf", "mpileup.6.tab", True),
    ("mpileup.5.vcf", "mpileup.7.tab", True),
    ("mpileup.cals.1.vcf", "mpileup.cals.1.tab", False),
    ("mpileup.cals.2.vcf", "mpileup.cals.2.tab", False),
]
R_KEYS = ("AD", "ADF", "ADR")


def paired(golden_dir, vcff, tab, ins, monkeypatch):
    """[(original Rec, target alleles, unseen, constrained Rec)] of every record the pairing hands to constrain_record and that is
    not skipped, and the file's Number=R FORMAT keys."""
    G = os.path.join(golden_dir, "call")
    vcf = V.Vcf(os.path.join(G, vcff))
    seen, inner = [], cals.constrain_record

    def spy(rec, tals, unseen, nsmpl, fmtR):
        r = inner(rec, tals, unseen, nsmpl, fmtR)
        if r is not None:
            seen.append((rec, tals, unseen, r[0]))
        return r
    monkeypatch.setattr(cals, "constrain_record", spy)
    cals.constrain(vcf, cals.parse_tab(os.path.join(G, tab)), ins)
    return seen, cals._numberR_formats(vcf.header)


def check_record(rec, tals, unseen, new):
    """The twin on the original record's planes against the planes of the constrained record's text; (changed, PL with '.', R keys)."""
    r = CP.descriptor(rec, tals, unseen, cals.Vcmp())
    assert r is not None
    d, nori = r
    site = np.array([d], dtype=CP.SITE_DTYPE)
    n_new = int(d["n_new"])
    assert n_new == len(new.alleles) and bool(d["changed"]) == (new is not rec)
    n_r = 0
    for extra in (0, 1):                                            # n_in / n_out at, and one above, what the record needs
        n_in, n_out = nori * (nori + 1) // 2 + extra, n_new * (n_new + 1) // 2 + extra
        got = CP.constrain(CP.text_planes(rec, "PL", n_in)[None], site, n_out, CP.NUMBER_G)[0]
        np.testing.assert_array_equal(got, CP.text_planes(new, "PL", n_out), err_msg="%s:%d PL" % (rec.chrom, rec.pos))
        for key in R_KEYS:
            if key not in rec.fmt_keys:
                continue
            n_r += 1 - extra
            got = CP.constrain(CP.text_planes(rec, key, nori + extra)[None], site, n_new + extra, CP.NUMBER_R)[0]
            np.testing.assert_array_equal(got, CP.text_planes(new, key, n_new + extra), err_msg="%s:%d %s" % (rec.chrom, rec.pos, key))
    dotted = any("." in (rec.fmt("PL", s) or "").split(",") for s in range(len(rec.smpl)))
    return bool(d["changed"]), dotted, n_r


@pytest.mark.parametrize("vcff,tab,ins", CALS_ROWS)
def test_twin_equals_the_record_rewrite(golden_dir, monkeypatch, vcff, tab, ins):
    seen, fmtR = paired(golden_dir, vcff, tab, ins, monkeypatch)
    assert seen
    n_changed = n_same = n_dotted = n_r_changed = 0
    for rec, tals, unseen, new in seen:
        changed, dotted, n_r = check_record(rec, tals, unseen, new)
        assert all(k in fmtR for k in R_KEYS if k in rec.fmt_keys)
        n_changed += changed
        n_same += not changed
        n_dotted += changed and dotted
        n_r_changed += changed and n_r > 0
    assert n_changed > 0                                            # every row has a record the rewrite changes
    if (vcff, tab) == ("mpileup.vcf", "mpileup.tab"):
        assert (n_changed, n_same, n_dotted) == (8, 3, 6)
    if vcff in ("mpileup.2.vcf", "mpileup.cals.1.vcf"):
        assert n_r_changed > 0                                      # a changed record with AD / ADF / ADR


def test_the_rule_on_small_vectors():
    """The cases no golden reaches, by hand: the three fallbacks in turn, `end of vector` cutting the rest, an amap entry past the
    input's planes, the single `.` of a Number=R vector, and a vector one value short."""
    M, E = CP.MISSING, CP.VEND
    d = np.zeros(1, CP.SITE_DTYPE)
    d["n_new"], d["unseen"], d["changed"], d["amap"] = 3, 2, 1, [0, 1, 2, 0, 0]
    # alleles 0, 1 and the unseen 2; genotypes 00 01 11 02 12 22; four samples
    p = np.array([[10, 10, 10, E], [M, M, M, 5], [30, 30, 30, 6], [41, M, M, 7], [50, 52, M, 8], [60, 61, 62, E]], np.int32)
    out = CP.constrain(p[None], d, 7, CP.NUMBER_G)[0]
    assert out[1].tolist() == [41, 52, 62, 5]                       # gt(ia, u), gt(ib, u), gt(u, u); a value that is there
    assert out[0].tolist() == [10, 10, 10, M] and out[:, 3].tolist() == [M, 5, 6, 7, 8, E, E]
    assert (out[6] == E).all()
    d["amap"][0, 1] = 7                                             # past n_in: `end of vector` from genotype 1 on
    out = CP.constrain(p[None], d, 6, CP.NUMBER_G)[0]
    assert out[0].tolist() == [10, 10, 10, M] and (out[1:] == E).all()
    d["unseen"] = -1                                                # no fallback: `missing` stays
    d["amap"][0, 1] = 1
    assert CP.constrain(p[None], d, 6, CP.NUMBER_G)[0][1].tolist() == [M, M, M, 5]
    r = np.array([[M, 3, 3, M], [E, 4, 4, 9], [E, 5, E, 8]], np.int32)
    d["amap"][0, :3] = [0, 2, 1]
    out = CP.constrain(r[None], d, 4, CP.NUMBER_R)[0]
    assert out.T.tolist() == [[M, E, E, E], [3, 5, 4, E], [3, M, 4, E], [M, 8, 9, E]]
    d["changed"] = 0
    assert CP.constrain(r[None], d, 4, CP.NUMBER_R)[0].T.tolist() == [[M, E, E, E], [3, 4, 5, E], [3, 4, E, E], [M, 9, 8, E]]
