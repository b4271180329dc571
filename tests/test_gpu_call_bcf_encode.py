"""bcfgpu_call_encode_bcf: FORMAT/GT, the trimmed FORMAT/PL and FORMAT/GQ of call records as BCF2 key blocks, made on the device
from the caller's planes in HBM.  Planes are made in numpy and uploaded; the bytes and all n * 3 + 1 offsets are compared exactly
with the numpy twin of tests/helpers/callenc.py (itself pinned against the host writer in tests/test_call_indiv_encoder.py).
The shapes are the smallest that reach every branch: 37 sites with nals_new cycling 1..5, and 1, 3, 64, 65 and 257 samples --
one lane, a partial wavefront, one wavefront, one past it, one past the 256-lane workgroup and past a slice of a 15-wide int32
PL."""
import ctypes as C
import os

import numpy as np
import pytest

from bcftools_amd import abi, engine, host
from bcftools_amd.lib import check
from tests.helpers import callenc

pytestmark = pytest.mark.gpu

MISSING, VEND = abi.INT32_MISSING, abi.INT32_VECTOR_END
IDS = {"GT": 9, "PL": 7, "GQ": 11}
N = 37
SIZES = [1, 3, 64, 65, 257]


def planes(rng, n, S, ploidy="diploid", hi=100):
    """A host CallResult of n called variant-or-not sites: nals_new cycles 1..5, ret = nals_new (0 at every seventh site), PL below
    `hi` over the first ngn planes (ploidy 1: the first nn) and VEND behind, GQ below hi.  ploidy: "diploid", "haploid", or the
    index of the single diploid sample among haploid ones."""
    res = host.CallResult(n, S, abi.MAX_PL)
    nn = 1 + np.arange(n) % 5
    res.site["nals_new"] = nn
    res.site["ret"] = np.where(np.arange(n) % 7 == 6, 0, nn)
    dip = np.ones(S, bool) if ploidy == "diploid" else np.zeros(S, bool)
    if isinstance(ploidy, int):
        dip[ploidy] = True
    res.pl[:] = VEND
    for k in range(n):
        a = int(nn[k])
        res.gt[k, 0] = rng.integers(0, a, S)
        res.gt[k, 1] = np.where(dip, rng.integers(0, a, S), abi.GT_VECTOR_END)
        res.pl[k, :a * (a + 1) // 2, dip] = rng.integers(0, hi, (int(dip.sum()), a * (a + 1) // 2))
        res.pl[k, :a, ~dip] = rng.integers(0, hi, (int((~dip).sum()), a))
    res.gq[:] = rng.integers(0, hi, res.gq.shape)
    return res


def upload(ctx, res, pl=True, gq=True):
    o = abi.CallOut()
    o.site, o.gt = ctx.to_device(res.site).ptr, ctx.to_device(res.gt).ptr
    if pl:
        o.pl = ctx.to_device(res.pl).ptr
    if gq:
        o.gq = ctx.to_device(res.gq).ptr
    return o


def want(res, ids=IDS, emit=None, pl=True, gq=True):
    return callenc.encode_planes(ids, res.site, res.gt, res.pl if pl else None, res.gq if gq else None, emit)


def check_equal(got, exp):
    data, off = got
    wdata, woff = exp
    assert len(off) == len(woff)
    np.testing.assert_array_equal(off, woff)
    assert data.tobytes() == wdata.tobytes()


def context(S, n=N):
    return engine.Context(abi.default_cfg(S, max_sites=max(n, 1), max_reads=64))


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("ploidy", ["diploid", "haploid", "first", "last", "middle"])
def test_every_ploidy_and_width(S, ploidy):
    """All diploid, all haploid (GT one wide, PL nals wide), one diploid sample among haploid ones; missing genotypes of both
    spellings, a sample whose PL is missing, dropped PL, sites that have no GQ; a third of the sites lifted to int16 / int32."""
    rng = np.random.default_rng(S)
    res = planes(rng, N, S, {"first": 0, "last": S - 1, "middle": S // 2}.get(ploidy, ploidy))
    for k in range(0, N, 3):
        s = int(rng.integers(0, S))
        res.pl[k, 0, s] = (200, 40000, 99999)[(k // 3) % 3]
    for k in range(1, N, 4):                                    # ./. or . (whatever the sample's ploidy), and its PL missing
        s = int(rng.integers(0, S))
        res.gt[k, 0, s] = abi.GT_MISSING
        if res.gt[k, 1, s] != abi.GT_VECTOR_END:
            res.gt[k, 1, s] = abi.GT_MISSING
        res.pl[k, :, s] = VEND
        res.pl[k, 0, s] = MISSING if k % 8 == 1 else VEND      # `missing` in plane 0, or a vector that ends at once
        res.gq[k, s] = MISSING
    res.site["pl_dropped"][5::11] = 1
    with context(S) as ctx:
        got = ctx.encode_call_bcf(upload(ctx, res), N, abi.MAX_PL, IDS)
    exp = want(res)
    check_equal(got, exp)
    starts = exp[1][:-1][np.diff(exp[1]) > 0]
    assert len({int(x) % 16 for x in starts}) > (2 if S == 1 else 6)               # the blocks start at many alignments
    if ploidy == "haploid":                                     # GT one wide: 2 + 1 + S bytes
        assert int(exp[1][1] - exp[1][0]) == 3 + S


@pytest.mark.parametrize("S", [3, 257])
def test_every_sample_missing(S):
    """No genotype and no PL in any sample: GT 0,0 (or 0), PL one `missing` a sample as int8, GQ missing."""
    res = planes(np.random.default_rng(1), N, S)
    res.gt[:, 0] = abi.GT_MISSING
    res.gt[::2, 1] = abi.GT_MISSING
    res.gt[1::2, 1] = abi.GT_VECTOR_END
    res.pl[:] = VEND
    res.pl[::3, 0] = MISSING
    res.gq[:] = MISSING
    with context(S) as ctx:
        got = ctx.encode_call_bcf(upload(ctx, res), N, abi.MAX_PL, IDS)
    check_equal(got, want(res))
    off = got[1]
    assert int(off[2] - off[1]) == 3 + S and int(off[3 + 2] - off[3 + 1]) == 3 + S


@pytest.mark.parametrize("S", [3, 65, 257])
def test_the_type_follows_a_single_samples_value(S):
    """PL's largest value at 127, 128, 32767, 32768 and 99 999 and its smallest at the negative bounds, held by one sample alone
    (first, last, middle) with sentinels in the others; GQ at 127 / 128 and 32767 / 32768."""
    bounds = [127, 128, 32767, 32768, 99999, -120, -121, -32760, -32761]
    cases = [(v, s) for v in bounds for s in (0, S - 1, S // 2)]
    n = len(cases)
    res = planes(np.random.default_rng(2), n, S, hi=50)
    for k, (v, s) in enumerate(cases):
        nn = int(res.site["nals_new"][k])
        res.pl[k, nn * (nn + 1) // 2 - 1, s] = v
        o = (s + 1) % S
        if o != s:
            res.pl[k, :, o] = VEND
            res.pl[k, 0, o] = MISSING
        if S > 2:
            res.pl[k, 1:, (s + 2) % S] = VEND                   # (one value, then the end; at nals_new 1 nothing changes)
        res.gq[k, s] = (127, 128, 32767, 32768)[k % 4]
        res.gq[k, o] = MISSING if o != s else res.gq[k, o]
    with context(S, n) as ctx:
        got = ctx.encode_call_bcf(upload(ctx, res), n, abi.MAX_PL, IDS)
    check_equal(got, want(res))


def test_a_null_gq_plane_and_a_null_pl_plane():
    S = 65
    res = planes(np.random.default_rng(5), N, S)
    with context(S) as ctx:
        check_equal(ctx.encode_call_bcf(upload(ctx, res, gq=False), N, abi.MAX_PL, IDS), want(res, gq=False))
        res.site["pl_dropped"] = 1
        check_equal(ctx.encode_call_bcf(upload(ctx, res, pl=False), N, abi.MAX_PL, IDS), want(res, pl=False))
        check_equal(ctx.encode_call_bcf(upload(ctx, res), N, abi.MAX_PL, IDS), want(res, pl=False))


def test_fewer_planes_than_fifteen():
    """n_gt_max = 6 (no site with more than three alleles): the planes are read with that stride."""
    S, n = 65, 12
    res = planes(np.random.default_rng(8), n, S)
    nn = 1 + np.arange(n) % 3
    res.site["nals_new"], res.site["ret"] = nn, nn
    small = host.CallResult(n, S, 6)
    small.site[:], small.gt[:], small.gq[:] = res.site, res.gt, res.gq
    small.pl[:] = VEND
    for k in range(n):
        g = int(nn[k]) * (int(nn[k]) + 1) // 2
        small.pl[k, :g] = res.pl[k, :g]
    with context(S, n) as ctx:
        check_equal(ctx.encode_call_bcf(upload(ctx, small), n, 6, IDS), want(small))


@pytest.mark.parametrize("ids", [(9, 7, 11), (127, 128, 300), (32767, 32768, 70000), (70000, 5, 128)])
def test_key_ids_of_one_two_and_four_bytes(ids):
    S = 65
    res = planes(np.random.default_rng(6), N, S, hi=300)
    with context(S) as ctx:
        check_equal(ctx.encode_call_bcf(upload(ctx, res), N, abi.MAX_PL, ids), want(res, ids))
        check_equal(ctx.encode_call_bcf(upload(ctx, res), N, abi.MAX_PL, dict(zip(abi.CALL_BCF_KEYS, ids))), want(res, ids))


def test_emit_masks_and_no_sites():
    S = 65
    res = planes(np.random.default_rng(3), N, S, hi=300)
    first, last = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    first[0], last[-1] = 1, 1
    with context(S) as ctx:
        o = upload(ctx, res)
        for emit in (None, np.zeros(N, np.uint8), np.ones(N, np.uint8), (np.arange(N) % 2).astype(np.uint8), first, last):
            check_equal(ctx.encode_call_bcf(o, N, abi.MAX_PL, IDS, emit=emit), want(res, emit=emit))
        data, off = ctx.encode_call_bcf(o, 0, abi.MAX_PL, IDS)
        assert len(data) == 0 and off.tolist() == [0]
    assert len(want(res, emit=np.zeros(N, np.uint8))[0]) == 0


def test_a_buffer_one_byte_short_is_left_alone():
    """cap_bytes one byte short: BCFGPU_E_RANGE, *n_bytes the size needed, nothing written; the exact size succeeds."""
    S = 65
    res = planes(np.random.default_rng(4), N, S, hi=300)
    wdata, woff = want(res)
    need = len(wdata)
    ids = (C.c_int32 * 3)(*[IDS[k] for k in abi.CALL_BCF_KEYS])
    with context(S) as ctx:
        o = upload(ctx, res)
        buf, off = ctx.buf(need), ctx.buf(8 * (N * 3 + 1))
        check(ctx.L.bcfgpu_memset(ctx.h, buf.ptr, 0xA5, need))
        nb = C.c_uint64(0)
        rc = ctx.L.bcfgpu_call_encode_bcf(ctx.h, N, abi.MAX_PL, C.byref(o), ids, None, buf.ptr, need - 1, off.ptr, C.byref(nb))
        assert rc == abi.E_RANGE and nb.value == need
        assert (buf.download(np.zeros(need, np.uint8)) == 0xA5).all()
        np.testing.assert_array_equal(off.download(np.zeros(N * 3 + 1, np.uint64)), woff)       # the offsets are set all the same
        with pytest.raises(engine.BcfGpuError) as e:
            ctx.encode_call_bcf(o, N, abi.MAX_PL, IDS, cap_bytes=need - 1)
        assert e.value.code == abi.E_RANGE and e.value.needed == need
        rc = ctx.L.bcfgpu_call_encode_bcf(ctx.h, N, abi.MAX_PL, C.byref(o), ids, None, None, 0, off.ptr, C.byref(nb))
        assert rc == abi.E_RANGE and nb.value == need                                           # cap_bytes = 0 asks for the size
        rc = ctx.L.bcfgpu_call_encode_bcf(ctx.h, N, abi.MAX_PL, C.byref(o), ids, None, buf.ptr, need, off.ptr, C.byref(nb))
        assert rc == 0 and nb.value == need
        assert buf.download(np.zeros(need, np.uint8)).tobytes() == wdata.tobytes()
        np.testing.assert_array_equal(off.download(np.zeros(N * 3 + 1, np.uint64)), woff)
        # bad arguments: no planes, a negative key id, a plane count outside 1 .. 15
        neg = (C.c_int32 * 3)(9, -1, 11)
        assert ctx.L.bcfgpu_call_encode_bcf(ctx.h, N, abi.MAX_PL, None, ids, None, buf.ptr, need, off.ptr, C.byref(nb)) == abi.E_ARG
        assert ctx.L.bcfgpu_call_encode_bcf(ctx.h, N, abi.MAX_PL, C.byref(o), neg, None, buf.ptr, need, off.ptr, C.byref(nb)) == abi.E_ARG
        assert ctx.L.bcfgpu_call_encode_bcf(ctx.h, N, 16, C.byref(o), ids, None, buf.ptr, need, off.ptr, C.byref(nb)) == abi.E_ARG
        assert ctx.L.bcfgpu_call_encode_bcf(ctx.h, N, 0, C.byref(o), ids, None, buf.ptr, need, off.ptr, C.byref(nb)) == abi.E_ARG


def test_planes_of_a_real_call(golden_dir):
    """The records of the X-chromosome golden (haploid males beside diploid females) through bcfgpu_mcall with GQ: the blocks made
    from the planes in HBM are the twin's over the downloaded planes, and the records are the golden's."""
    from tests.helpers import calldrv as D, vcf
    G = os.path.join(golden_dir, "call")
    seen = []

    def eng(cfg, cin):
        with engine.Context(cfg) as ctx:
            o, ob, res = ctx.mcall_device(cin)
            emit = (res.site["ret"] > 0).astype(np.uint8)
            got = ctx.encode_call_bcf(o, cin.n_sites, cin.n_gt_max, IDS, emit=emit)
            check_equal(got, callenc.encode_planes(IDS, res.site, res.gt, res.pl, res.gq, emit))
            seen.append((len(got[0]), int(emit.sum()), bool((res.gt[:, 1] == abi.GT_VECTOR_END).any())))
        return res
    called, names = D.run_call(vcf.Vcf(os.path.join(G, "mpileup.X.vcf")), eng, call_flag=abi.CALL_VARONLY, output_tags=abi.CALL_FMT_GQ,
                               samples=D.parse_samples_file(os.path.join(G, "mpileup.samples")),
                               ploidy=D.parse_ploidy_file(os.path.join(G, "mpileup.ploidy")))
    D.compare_with_golden(called, names, vcf.Vcf(os.path.join(G, "mpileup.X.out")))
    assert seen and sum(s[1] for s in seen) >= len(called) > 0 and any(s[2] for s in seen) and all(s[0] > 0 for s in seen if s[1])
