"""bcfgpu_mplp_encode_vcf: the sample columns of every mpileup record of a tile as VCF text, made on the device from the result
planes in HBM.  Planes are made in numpy and uploaded; bytes and offsets are compared exactly with the Python encoder of
tests/helpers/vcfenc.py (itself pinned to the reference's goldens in tests/test_vcf_sample_text.py).  The shapes are the
smallest that reach every branch: one lane, a partial wavefront, one wavefront, one past it, past a 256-lane workgroup; every
PL width; every digit count per key with the deciding value in a single sample; rounds cut by the stage's bytes in the middle
of a workgroup; NULL planes; blocks that start at any byte."""
import ctypes as C
import os

import numpy as np
import pytest

from bcftools_amd import abi, engine, host
from bcftools_amd.lib import check
from tests.helpers import vcfenc

pytestmark = pytest.mark.gpu

ALL_FMT = abi.FMT_DP | abi.FMT_DV | abi.FMT_SP | abi.FMT_DP4 | abi.FMT_ADF | abi.FMT_ADR | abi.FMT_AD | abi.FMT_DPR | abi.FMT_SCR | abi.FMT_QS
PLANES = ("pl", "dp4", "adf", "adr", "qs", "scr", "sp")


def mixed_planes(rng, n, S):
    """A host MplpResult with n_alleles cycling 1..5 and values of every digit count their planes hold: the exponent is drawn
    first, so that one-digit values are as frequent as the longest."""
    res = host.MplpResult(n, S)
    res.site["n_alleles"] = 1 + np.arange(n) % 5

    def draw(shape, top):
        return np.minimum((10.0 ** rng.uniform(0, np.log10(top + 1.0), shape)).astype(np.int64) - (rng.random(shape) < 0.2), top).clip(0)

    res.pl[:] = draw(res.pl.shape, 255)
    res.sp[:] = draw(res.sp.shape, 255)
    for name in ("dp4", "adf", "adr", "scr"):
        getattr(res, name)[:] = draw(getattr(res, name).shape, 65535)
    res.qs[:] = draw(res.qs.shape, 2147483647)
    return res


def max_planes(n, S, na=5):
    res = host.MplpResult(n, S)
    res.site["n_alleles"] = na
    res.pl[:], res.sp[:], res.qs[:] = 255, 255, 2147483647
    for name in ("dp4", "adf", "adr", "scr"):
        getattr(res, name)[:] = 65535
    return res


def upload(ctx, res, names=PLANES):
    """abi.MplpOut of device copies of the named planes (the others NULL) and the site records."""
    o = abi.MplpOut()
    o.site = ctx.to_device(res.site).ptr
    for k in names:
        setattr(o, k, ctx.to_device(getattr(res, k)).ptr)
    return o


def want(fmt, res, emit=None):
    return vcfenc.encode_planes(fmt, res.site["n_alleles"], res.pl, res.dp4, res.adf, res.adr, res.qs, res.scr, res.sp, emit)


def check_equal(got, exp):
    data, off = got
    wdata, woff = exp
    np.testing.assert_array_equal(off, woff)
    assert data.tobytes() == wdata.tobytes()


def poke(res, key, k, s, v):
    """Value v in `key` at site k, sample s (the last value of the key; the sums split over their planes)."""
    na = int(res.site["n_alleles"][k])
    if key == "PL":
        res.pl[k, na * (na + 1) // 2 - 1, s] = v
    elif key == "SP":
        res.sp[k, s] = v
    elif key == "DP":                         # the sum of the four planes
        res.dp4[k, :, s] = [v // 4, v // 4, v // 4, v - 3 * (v // 4)]
    elif key == "DV":
        res.dp4[k, 2:, s] = [v // 2, v - v // 2]
    elif key in ("AD", "DPR"):                # ADF + ADR
        res.adf[k, na - 1, s], res.adr[k, na - 1, s] = v // 2, v - v // 2
    elif key == "QS":
        res.qs[k, na - 1, s] = v
    elif key == "DP4":
        res.dp4[k, 1, s] = v
    elif key == "SCR":
        res.scr[k, s] = v
    else:
        getattr(res, key.lower())[k, na - 1, s] = v


@pytest.mark.parametrize("S", [1, 3, 64, 65, 257])
def test_all_keys_every_width(S):
    """37 sites, n_alleles 1..5 (PL widths 1, 3, 6, 10, 15), all eleven keys, values of mixed digit counts: blocks of every
    size follow each other and start at every alignment."""
    n = 37
    res = mixed_planes(np.random.default_rng(S), n, S)
    with engine.Context(abi.default_cfg(S, max_sites=n, max_reads=64, fmt_flag=ALL_FMT)) as ctx:
        got = ctx.encode_vcf(upload(ctx, res), n)
    exp = want(ALL_FMT, res)
    check_equal(got, exp)
    assert len({int(x) % 16 for x in exp[1][:-1]}) > 8                          # the blocks start at many residues mod 16
    lens = {len(str(int(v))) for v in res.qs[:, 0].ravel()}
    assert lens == set(range(1, 11)) or S < 64


BOUNDS = {"PL": (9, 10, 99, 100, 255), "SP": (9, 10, 99, 100, 255),
          "DP4": (999, 1000, 9999, 10000, 65535), "ADF": (999, 1000, 9999, 10000, 65535), "ADR": (999, 1000, 9999, 10000, 65535),
          "SCR": (999, 1000, 9999, 10000, 65535), "DV": (999, 1000, 9999, 10000, 65535),
          "DP": (99999, 100000, 262140), "AD": (131070,), "DPR": (131070,), "QS": (999999999, 1000000000, 2147483647)}


def test_digit_boundaries_per_key():
    """Per key a value on either side of a digit boundary and the largest its planes give, in one sample only -- the first, the
    last or a middle one -- with everything else zero.  DP reaches six digits with each DP4 plane at five; AD and DPR with ADF
    and ADR at 65535 each."""
    S = 65
    assert set(BOUNDS) == set(abi.BCF_KEYS)
    cases = [(key, v, s) for key in abi.BCF_KEYS for v in BOUNDS[key] for s in (0, S // 2, S - 1)]
    res = host.MplpResult(len(cases), S)
    res.site["n_alleles"] = 1 + np.arange(len(cases)) % 5
    for k, (key, v, s) in enumerate(cases):
        poke(res, key, k, s, v)
    k_dp = cases.index(("DP", 262140, 0))
    assert (res.dp4[k_dp, :, 0] == 65535).all()
    k_ad = cases.index(("AD", 131070, S - 1))
    assert res.adf[k_ad, :, S - 1].max() == 65535 == res.adr[k_ad, :, S - 1].max()
    with engine.Context(abi.default_cfg(S, max_sites=len(cases), max_reads=64, fmt_flag=ALL_FMT)) as ctx:
        got = ctx.encode_vcf(upload(ctx, res), len(cases))
    exp = want(ALL_FMT, res)
    check_equal(got, exp)
    text = exp[0].tobytes()
    for key, v, s in cases:                                                     # the twin did print them
        assert b"%d" % v in text


def test_rounds_are_cut_by_the_stage_not_by_a_sample_count():
    """S = 257 with every value at its plane's maximum: 256 samples of 293 bytes are nearly five stages, so a round ends after
    52 samples; then all-zero and all-maximum samples alternating, so that the cut falls at other lanes; then site after site
    with another sample long, so that the cut moves lane by lane."""
    S = 257
    top = max_planes(3, S)
    top.site["n_alleles"] = [5, 3, 1]
    alt = max_planes(2, S)
    for name in PLANES:
        getattr(alt, name)[..., 0::2] = 0
    alt.site["n_alleles"] = [5, 4]
    rng = np.random.default_rng(11)
    mix = max_planes(6, S)
    for k in range(6):
        zero = rng.random(S) < 0.1 * (k + 1)
        for name in PLANES:
            getattr(mix, name)[k][..., zero] = 0
    with engine.Context(abi.default_cfg(S, max_sites=8, max_reads=64, fmt_flag=ALL_FMT)) as ctx:
        for res in (top, alt, mix):
            n = len(res.site)
            exp = want(ALL_FMT, res)
            first = int(exp[1][1])
            assert first > 2 * vcfenc.STAGE and first // S < vcfenc.SAMPLE_MAX + 1      # more than one stage in the first 256 samples
            check_equal(ctx.encode_vcf(upload(ctx, res), n), exp)
    assert int(want(ALL_FMT, top)[1][1]) == S * vcfenc.SAMPLE_MAX and 256 * vcfenc.SAMPLE_MAX > 4 * vcfenc.STAGE


@pytest.mark.parametrize("fmt,names", [
    (0, ("pl",)),
    (abi.FMT_DP, ("pl", "dp4")),
    (abi.FMT_AD, ("pl", "adf", "adr")),
    (abi.FMT_SP | abi.FMT_DP4, ("pl", "sp", "dp4")),
    (abi.FMT_SCR | abi.FMT_QS, ("pl", "scr", "qs")),
    (abi.FMT_ADF | abi.FMT_DV | abi.FMT_DPR, ("pl", "adf", "adr", "dp4")),
])
def test_flag_subsets_with_null_planes(fmt, names):
    """Only PL and the keys the context's fmt_flag selects are written; the planes no selected key reads are NULL."""
    S, n = 65, 37
    res = mixed_planes(np.random.default_rng(fmt + 1), n, S)
    with engine.Context(abi.default_cfg(S, max_sites=n, max_reads=64, fmt_flag=fmt)) as ctx:
        got = ctx.encode_vcf(upload(ctx, res, names), n)
    check_equal(got, want(fmt, res))


def test_a_missing_plane_is_an_error():
    S, n = 3, 2
    res = mixed_planes(np.random.default_rng(5), n, S)
    with engine.Context(abi.default_cfg(S, max_sites=n, max_reads=64, fmt_flag=abi.FMT_AD)) as ctx:
        with pytest.raises(engine.BcfGpuError) as e:
            ctx.encode_vcf(upload(ctx, res, ("pl", "adf")), n)
        assert e.value.code == abi.E_ARG


def test_emit_masks_and_an_empty_tile():
    S, n = 65, 37
    fmt = abi.FMT_DP | abi.FMT_AD
    res = mixed_planes(np.random.default_rng(3), n, S)
    first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    first[0], last[-1] = 1, 1
    with engine.Context(abi.default_cfg(S, max_sites=n, max_reads=64, fmt_flag=fmt)) as ctx:
        o = upload(ctx, res)
        for emit in (None, np.zeros(n, np.uint8), (np.arange(n) % 2).astype(np.uint8), first, last):
            check_equal(ctx.encode_vcf(o, n, emit=emit), want(fmt, res, emit))
        data, off = ctx.encode_vcf(o, 0)
        assert len(data) == 0 and off.tolist() == [0]
    assert len(want(fmt, res, np.zeros(n, np.uint8))[0]) == 0


def test_a_buffer_one_byte_short_is_left_alone():
    """cap_bytes one byte short: BCFGPU_E_RANGE, *n_bytes the size needed, nothing written; the exact size succeeds."""
    S, n = 65, 37
    res = mixed_planes(np.random.default_rng(4), n, S)
    wdata, woff = want(ALL_FMT, res)
    need = len(wdata)
    with engine.Context(abi.default_cfg(S, max_sites=n, max_reads=64, fmt_flag=ALL_FMT)) as ctx:
        o = upload(ctx, res)
        buf, off = ctx.buf(need), ctx.buf(8 * (n + 1))
        check(ctx.L.bcfgpu_memset(ctx.h, buf.ptr, 0xA5, need))
        nb = C.c_uint64(0)
        rc = ctx.L.bcfgpu_mplp_encode_vcf(ctx.h, n, C.byref(o), None, buf.ptr, need - 1, off.ptr, C.byref(nb))
        assert rc == abi.E_RANGE and nb.value == need
        back = buf.download(np.zeros(need, np.uint8))
        assert (back == 0xA5).all()
        np.testing.assert_array_equal(off.download(np.zeros(n + 1, np.uint64)), woff)       # set whether or not the blocks fit
        with pytest.raises(engine.BcfGpuError) as e:
            ctx.encode_vcf(o, n, cap_bytes=need - 1)
        assert e.value.code == abi.E_RANGE and e.value.needed == need
        rc = ctx.L.bcfgpu_mplp_encode_vcf(ctx.h, n, C.byref(o), None, buf.ptr, need, off.ptr, C.byref(nb))
        assert rc == 0 and nb.value == need
        assert buf.download(np.zeros(need, np.uint8)).tobytes() == wdata.tobytes()
        np.testing.assert_array_equal(off.download(np.zeros(n + 1, np.uint64)), woff)


def test_planes_of_real_tiles_both_passes(golden_dir):
    """A small tile of the reference's fixtures through bcfgpu_mpileup, the SNP pass and the indel pass (the insertion at
    17:302 of mpileup.2.out): the text made from the planes in HBM is the Python encoder's over the downloaded planes."""
    from tests.helpers import mplpdrv as M, sam
    G = os.path.join(golden_dir, "mpileup")
    fmt = abi.INFO_VDB | abi.INFO_RPB | abi.FMT_DP | abi.FMT_DV | abi.FMT_AD | abi.FMT_SP | abi.FMT_DP4
    sams = [sam.Sam(os.path.join(G, "mpileup.%d.sam" % i)) for i in (1, 2, 3)]
    prep = M.Prepared(sams, sam.read_fasta(os.path.join(G, "mpileup.ref.fa")), "17", sam.MplpOpts(fmt_flag=fmt))
    snp, _, kept = M.snp_tile(prep, range(280, 330))
    per = M.column(prep, 301)
    g = M.gap_prep(prep, per, 301)
    assert g is not None and len(kept) == 50
    tiles = [snp, M.indel_tile(prep, per, g)]
    S = len(prep.samples)
    with engine.Context(abi.default_cfg(S, max_sites=64, max_reads=1 << 16, fmt_flag=fmt)) as ctx:
        for t in tiles:
            dt, tb = ctx.upload_tile(t)
            o, ob, res = ctx.alloc_mplp_out(t.n_sites)
            for b in ob.values():
                check(ctx.L.bcfgpu_memset(ctx.h, b.ptr, 0, b.nbytes))
            check(ctx.L.bcfgpu_mpileup(ctx.h, C.byref(dt), C.byref(o)))
            ctx.sync()
            ctx._download(ob, res)
            emit = (res.site["ret"] == 0).astype(np.uint8)
            assert emit.all() and res.site["n_alleles"].max() >= 2
            got = ctx.encode_vcf(o, t.n_sites, emit=emit)
            check_equal(got, want(fmt, res, emit))
            assert len(got[0]) > 10 * S * t.n_sites
            ctx.release(tb + list(ob.values()))
