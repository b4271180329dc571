"""tests/helpers/vcfenc.py, the CPU twin of bcfgpu_mplp_encode_vcf, pinned to the reference: for every record of the goldens the
FORMAT values are parsed from the line, turned into result planes, and the twin's block must be the line's own bytes from the
tab after the FORMAT column to the end of the line.  Then known answers at the seams: every digit count, one key and eleven,
one allele and five, an emit mask.  CPU only."""
import os

import numpy as np
import pytest

from bcftools_amd import abi
from tests.helpers import vcfenc

GOLDENS = ("mpileup.2.out", "mpileup.4.out", "mpileup.5.out", "mpileup.11.out", "indel-AD.1.out", "mpileup-SCR.out")
FLAG = dict(zip(abi.BCF_KEYS, abi.BCF_KEY_FLAG))
ALL_FMT = sum(abi.BCF_KEY_FLAG)


def planes_of(keys, na, samples):
    """One site's planes ([1][plane][S]) that give back the FORMAT values of a record: samples = [{key: [values]}]."""
    S = len(samples)
    pl, dp4 = np.zeros((1, abi.MAX_PL, S), np.uint8), np.zeros((1, 4, S), np.uint16)
    adf, adr = np.zeros((1, 5, S), np.uint16), np.zeros((1, 5, S), np.uint16)
    qs, scr, sp = np.zeros((1, 5, S), np.int32), np.zeros((1, S), np.uint16), np.zeros((1, S), np.uint8)
    for s, v in enumerate(samples):
        assert len(v["PL"]) == na * (na + 1) // 2
        pl[0, :len(v["PL"]), s] = v["PL"]
        if "DP4" in keys:
            dp4[0, :, s] = v["DP4"]
        else:                                           # DP = the sum of the four counts, DV = the last two
            dv = v["DV"][0] if "DV" in keys else 0
            dp = v["DP"][0] if "DP" in keys else dv
            dp4[0, :, s] = [dp - dv, 0, dv, 0]
        for key in ("AD", "DPR"):                       # AD = DPR = ADF + ADR
            if key in keys and "ADF" not in keys:
                adf[0, :na, s] = v[key]
        if "ADF" in keys:
            adf[0, :na, s], adr[0, :na, s] = v["ADF"], v["ADR"]
        if "QS" in keys:
            qs[0, :na, s] = v["QS"]
        if "SCR" in keys:
            scr[0, s] = v["SCR"][0]
        if "SP" in keys:
            sp[0, s] = v["SP"][0]
    return pl, dp4, adf, adr, qs, scr, sp


@pytest.mark.parametrize("goldf", GOLDENS)
def test_the_twin_writes_the_goldens_sample_columns(golden_dir, goldf):
    n = 0
    for ln in open(os.path.join(golden_dir, "mpileup", goldf), "rb").read().split(b"\n"):
        if not ln or ln.startswith(b"#"):
            continue
        f = ln.split(b"\t")
        keys = f[8].decode().split(":")
        assert keys == [k for k in abi.BCF_KEYS if k in keys] and keys[0] == "PL"        # the order of BCFGPU_BCF_*
        na = 1 if f[4] == b"." else 2 + f[4].count(b",")
        samples = [{k: [int(x) for x in col.split(b",")] for k, col in zip(keys, c.split(b":"))} for c in f[9:]]
        fmt = sum(FLAG[k] for k in keys)
        data, off = vcfenc.encode_planes(fmt, [na], *planes_of(keys, na, samples))
        want = ln[len(b"\t".join(f[:9])):]
        assert want[:1] == b"\t" and data.tobytes() == want, ln
        assert off.tolist() == [0, len(want)]
        n += 1
    assert n >= 86


SEAMS = (0, 9, 10, 99, 100, 65535, 99999, 100000, 2147483647)


def test_known_answers_one_key():
    """QS alone beside PL would still be two keys: one key is PL, whose plane holds 0..255."""
    pl = np.zeros((2, abi.MAX_PL, 3), np.uint8)
    pl[0, 0] = [0, 9, 10]
    pl[1, :3, 0], pl[1, :3, 1], pl[1, :3, 2] = [99, 100, 255], [0, 0, 0], [10, 9, 100]
    dp4 = np.zeros((2, 4, 3), np.uint16)
    data, off = vcfenc.encode_planes(0, [1, 2], pl, dp4)
    assert data.tobytes() == b"\t0\t9\t10" + b"\t99,100,255\t0,0,0\t10,9,100"
    assert off.tolist() == [0, 7, 33]


def test_known_answers_every_digit_count():
    """PL:QS of one allele, a sample per seam value: QS is the int32 plane and holds all of them."""
    S = len(SEAMS)
    pl, dp4, qs = np.zeros((1, abi.MAX_PL, S), np.uint8), np.zeros((1, 4, S), np.uint16), np.zeros((1, 5, S), np.int32)
    qs[0, 0] = SEAMS
    data, off = vcfenc.encode_planes(abi.FMT_QS, [1], pl, dp4, qs=qs)
    want = b"\t0:0\t0:9\t0:10\t0:99\t0:100\t0:65535\t0:99999\t0:100000\t0:2147483647"
    assert data.tobytes() == want and off.tolist() == [0, len(want)]


def test_known_answers_eleven_keys_five_alleles_and_a_mask():
    """All eleven keys: a site of one allele, a masked site, a site of five alleles; DP, DV, AD and DPR are sums."""
    S = 2
    pl, dp4 = np.zeros((3, abi.MAX_PL, S), np.uint8), np.zeros((3, 4, S), np.uint16)
    adf, adr = np.zeros((3, 5, S), np.uint16), np.zeros((3, 5, S), np.uint16)
    qs, scr, sp = np.zeros((3, 5, S), np.int32), np.zeros((3, S), np.uint16), np.zeros((3, S), np.uint8)
    dp4[0, :, 0] = [65535, 65535, 65535, 65535]
    adf[0, 0, 0], adr[0, 0, 0], scr[0, 0], sp[0, 0], qs[0, 0, 0], pl[0, 0, 0] = 65535, 65535, 65535, 255, 2147483647, 255
    pl[1] = 77                                                    # masked: nothing of it may show
    pl[2, :, 1] = np.arange(15) * 17
    dp4[2, :, 1] = [9, 10, 99, 100]
    adf[2, :, 1], adr[2, :, 1] = [1, 20, 300, 4000, 50000], [9, 80, 700, 6000, 50000]
    qs[2, :, 1] = [99999, 100000, 0, 9, 10]
    scr[2, 1], sp[2, 1] = 100, 99
    emit = np.array([1, 0, 1], np.uint8)
    data, off = vcfenc.encode_planes(ALL_FMT, [1, 3, 5], pl, dp4, adf, adr, qs, scr, sp, emit)
    site0 = (b"\t255:262140:131070:255:65535,65535,65535,65535:65535:65535:131070:131070:65535:2147483647"
             b"\t0:0:0:0:0,0,0,0:0:0:0:0:0:0")
    zeros5 = b"0,0,0,0,0"
    site2 = (b"\t" + b",".join([b"0"] * 15) + b":0:0:0:0,0,0,0:" + b":".join([zeros5] * 4) + b":0:" + zeros5 +
             b"\t0,17,34,51,68,85,102,119,136,153,170,187,204,221,238:218:199:99:9,10,99,100"
             b":1,20,300,4000,50000:9,80,700,6000,50000:10,100,1000,10000,100000:10,100,1000,10000,100000:100:99999,100000,0,9,10")
    assert data.tobytes() == site0 + site2
    assert off.tolist() == [0, len(site0), len(site0), len(site0) + len(site2)]
    full, _ = vcfenc.encode_planes(ALL_FMT, [1, 3, 5], pl, dp4, adf, adr, qs, scr, sp)
    assert full.tobytes()[len(site0):len(site0) + 7] == b"\t77,77,"


def test_the_worst_case_sample_is_what_the_kernel_states():
    """Every plane at its largest value, five alleles, eleven keys: the sample length vcfenc.hip asserts its stage against."""
    pl, dp4 = np.full((1, abi.MAX_PL, 1), 255, np.uint8), np.full((1, 4, 1), 65535, np.uint16)
    adf, adr = np.full((1, 5, 1), 65535, np.uint16), np.full((1, 5, 1), 65535, np.uint16)
    qs, scr, sp = np.full((1, 5, 1), 2147483647, np.int32), np.full((1, 1), 65535, np.uint16), np.full((1, 1), 255, np.uint8)
    data, _ = vcfenc.encode_planes(ALL_FMT, [5], pl, dp4, adf, adr, qs, scr, sp)
    assert len(data) == vcfenc.SAMPLE_MAX <= vcfenc.STAGE
    src = open(os.path.join(os.path.dirname(__file__), "..", "bcftools_amd", "csrc", "vcfenc.hip")).read()
    assert "VCF_SAMPLE_MAX == %d" % vcfenc.SAMPLE_MAX in src and "VCF_STAGE = 15 * 1024" in src and vcfenc.STAGE == 15 * 1024
