"""bcfgpu_mplp_encode_bcf: the per-sample part of every mpileup record of a tile as BCF2 bytes, made on the device from the
result planes in HBM.  Planes are made in numpy and uploaded; bytes and offsets are compared exactly with the numpy encoder
of tests/helpers/bcfenc.py (itself pinned against the host writer in tests/test_bcf_indiv_encoder.py).  The shapes are the
smallest that reach every branch: one lane, a partial wavefront, one wavefront, one past it, past a 256-lane workgroup;
every PL width; every integer type per key with the deciding value in a single sample; NULL planes; blocks that start at
any byte (the offsets of 37 sites of mixed sizes are odd and even alike)."""
import ctypes as C
import os

import numpy as np
import pytest

from bcftools_amd import abi, engine, host
from bcftools_amd.lib import check
from tests.helpers import bcfenc

pytestmark = pytest.mark.gpu

ALL_FMT = abi.FMT_DP | abi.FMT_DV | abi.FMT_SP | abi.FMT_DP4 | abi.FMT_ADF | abi.FMT_ADR | abi.FMT_AD | abi.FMT_DPR | abi.FMT_SCR | abi.FMT_QS
IDS = {k: 5 + i for i, k in enumerate(abi.BCF_KEYS)}
PLANES = ("pl", "dp4", "adf", "adr", "qs", "scr", "sp")


def small_planes(rng, n, S, hi=100):
    """A host MplpResult with n_alleles cycling 1..5 and every value below `hi`."""
    res = host.MplpResult(n, S)
    res.site["n_alleles"] = 1 + np.arange(n) % 5
    res.pl[:] = rng.integers(0, hi, res.pl.shape)
    res.dp4[:] = rng.integers(0, hi // 4, res.dp4.shape)
    res.adf[:] = rng.integers(0, hi // 2, res.adf.shape)
    res.adr[:] = rng.integers(0, hi // 2, res.adr.shape)
    res.qs[:] = rng.integers(0, hi, res.qs.shape)
    res.scr[:] = rng.integers(0, hi, res.scr.shape)
    res.sp[:] = rng.integers(0, hi, res.sp.shape)
    return res


def upload(ctx, res, names=PLANES):
    """abi.MplpOut of device copies of the named planes (the others NULL) and the site records."""
    o = abi.MplpOut()
    o.site = ctx.to_device(res.site).ptr
    for k in names:
        setattr(o, k, ctx.to_device(getattr(res, k)).ptr)
    return o


def want(fmt, ids, res, emit=None):
    return bcfenc.encode_planes(fmt, ids, res.site["n_alleles"], res.pl, res.dp4, res.adf, res.adr, res.qs, res.scr, res.sp, emit)


def check_equal(got, exp):
    data, off = got
    wdata, woff = exp
    np.testing.assert_array_equal(off, woff)
    assert data.tobytes() == wdata.tobytes()


def poke(res, key, k, s, v):
    """Make value v the largest of `key` at site k, held by sample s alone (as far as the plane's type allows: else False)."""
    na = int(res.site["n_alleles"][k])
    if key == "PL":
        if v > 255:
            return False
        res.pl[k, na * (na + 1) // 2 - 1, s] = v
    elif key == "SP":
        if v > 255:
            return False
        res.sp[k, s] = v
    elif key == "DP":                         # the sum of the four planes
        if v > 4 * 65535:
            return False
        res.dp4[k, :, s] = [v // 4, v // 4, v // 4, v - 3 * (v // 4)]
    elif key == "DV":
        if v > 2 * 65535:
            return False
        res.dp4[k, 2:, s] = [v // 2, v - v // 2]
    elif key in ("AD", "DPR"):                # ADF + ADR, each part below the sum's boundary
        if v > 2 * 65535:
            return False
        res.adf[k, na - 1, s], res.adr[k, na - 1, s] = v // 2, v - v // 2
    elif key == "QS":
        res.qs[k, na - 1, s] = v
    else:
        if v > 65535:
            return False
        if key == "DP4":
            res.dp4[k, 1, s] = v
        elif key == "SCR":
            res.scr[k, s] = v
        else:
            getattr(res, key.lower())[k, na - 1, s] = v
    return True


@pytest.mark.parametrize("S", [1, 3, 64, 65, 257])
def test_all_keys_every_width(S):
    """37 sites, n_alleles 1..5 (PL widths 1, 3, 6, 10, 15), all eleven keys; a third of the sites carry a value that lifts
    a key to int16 or int32, so that blocks of every size follow each other and start at every alignment."""
    rng = np.random.default_rng(S)
    n = 37
    res = small_planes(rng, n, S)
    for k in range(0, n, 3):
        key = abi.BCF_KEYS[(k // 3) % len(abi.BCF_KEYS)]
        poke(res, key, k, int(rng.integers(0, S)), (200, 40000, 70000)[(k // 3) % 3])
    with engine.Context(abi.default_cfg(S, max_sites=n, max_reads=64, fmt_flag=ALL_FMT)) as ctx:
        got = ctx.encode_bcf(upload(ctx, res), n, IDS)
    exp = want(ALL_FMT, IDS, res)
    check_equal(got, exp)
    assert len({int(x) % 16 for x in exp[1][:-1]}) > (1 if S == 1 else 4)          # the blocks start at many alignments


def test_type_boundaries_per_key():
    """Per key the largest value of a site at 127, 128, 255, 32767, 32768 and above, in one sample only -- the first, the
    last or a middle one -- with everything else zero.  AD and DPR straddle 32767 with ADF and ADR each below it; DP passes
    65535 with each DP4 plane below it."""
    S = 65
    bounds = (127, 128, 255, 32767, 32768, 70000, 262140)
    cases = [(key, v, s) for key in abi.BCF_KEYS for v in bounds for s in (0, S - 1, S // 2)]
    res = host.MplpResult(len(cases), S)
    res.site["n_alleles"] = 1 + np.arange(len(cases)) % 5
    reached = {}
    for k, (key, v, s) in enumerate(cases):
        if poke(res, key, k, s, v):
            reached.setdefault(key, set()).add(v)
    for key in abi.BCF_KEYS:                                    # every type of every key that its planes can hold
        top = 255 if key in ("PL", "SP") else 65535 if key in ("DP4", "ADF", "ADR", "SCR") else 262140 if key == "DP" else 70000
        assert reached[key] == {v for v in bounds if v <= top or (key == "QS")}, key
    k_ad = cases.index(("AD", 32768, S // 2))
    assert res.adf[k_ad].max() < 32767 and res.adr[k_ad].max() < 32767 and int(res.adf[k_ad].max()) + int(res.adr[k_ad].max()) == 32768
    k_dp = cases.index(("DP", 262140, 0))
    assert res.dp4[k_dp].max() == 65535
    k_dp = cases.index(("DP", 70000, 0))
    assert res.dp4[k_dp].max() < 32767 and res.dp4[k_dp, :, 0].sum() > 65535
    with engine.Context(abi.default_cfg(S, max_sites=len(cases), max_reads=64, fmt_flag=ALL_FMT)) as ctx:
        got = ctx.encode_bcf(upload(ctx, res), len(cases), IDS)
    check_equal(got, want(ALL_FMT, IDS, res))


@pytest.mark.parametrize("fmt,names,ids", [
    (0, ("pl",), (5,)),
    (abi.FMT_DP, ("pl", "dp4"), (127, 128)),
    (abi.FMT_AD, ("pl", "adf", "adr"), (300, 5)),
    (abi.FMT_SP | abi.FMT_DP4, ("pl", "sp", "dp4"), (128, 300, 127)),
    (abi.FMT_SCR | abi.FMT_QS, ("pl", "scr", "qs"), (40000, 127, 128)),
])
def test_flag_subsets_with_null_planes_and_key_ids(fmt, names, ids):
    """Only PL and the keys the context's fmt_flag selects are written; the planes no selected key reads are NULL.  Key ids
    of one, two and four bytes."""
    S, n = 65, 37
    res = small_planes(np.random.default_rng(fmt + 1), n, S, hi=400 if fmt & abi.FMT_QS else 100)
    keys = bcfenc.selected_keys(fmt)
    key_id = dict(zip(keys, ids))
    assert len(keys) == len(ids)
    with engine.Context(abi.default_cfg(S, max_sites=n, max_reads=64, fmt_flag=fmt)) as ctx:
        got = ctx.encode_bcf(upload(ctx, res, names), n, key_id)
    check_equal(got, want(fmt, key_id, res))


def test_emit_masks_and_an_empty_tile():
    S, n = 65, 37
    fmt = abi.FMT_DP | abi.FMT_AD
    res = small_planes(np.random.default_rng(3), n, S, hi=300)
    first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    first[0], last[-1] = 1, 1
    with engine.Context(abi.default_cfg(S, max_sites=n, max_reads=64, fmt_flag=fmt)) as ctx:
        o = upload(ctx, res)
        for emit in (None, np.zeros(n, np.uint8), (np.arange(n) % 2).astype(np.uint8), first, last):
            check_equal(ctx.encode_bcf(o, n, IDS, emit=emit), want(fmt, IDS, res, emit))
        data, off = ctx.encode_bcf(o, 0, IDS)
        assert len(data) == 0 and off.tolist() == [0]
    assert len(want(fmt, IDS, res, np.zeros(n, np.uint8))[0]) == 0


def test_a_buffer_one_byte_short_is_left_alone():
    """cap_bytes one byte short: BCFGPU_E_RANGE, *n_bytes the size needed, nothing written; the exact size succeeds."""
    S, n = 65, 37
    res = small_planes(np.random.default_rng(4), n, S, hi=300)
    wdata, woff = want(ALL_FMT, IDS, res)
    need = len(wdata)
    ids = (C.c_int32 * len(abi.BCF_KEYS))(*[IDS[k] for k in abi.BCF_KEYS])
    with engine.Context(abi.default_cfg(S, max_sites=n, max_reads=64, fmt_flag=ALL_FMT)) as ctx:
        o = upload(ctx, res)
        buf, off = ctx.buf(need), ctx.buf(8 * (n + 1))
        check(ctx.L.bcfgpu_memset(ctx.h, buf.ptr, 0xA5, need))
        nb = C.c_uint64(0)
        rc = ctx.L.bcfgpu_mplp_encode_bcf(ctx.h, n, C.byref(o), ids, None, buf.ptr, need - 1, off.ptr, C.byref(nb))
        assert rc == abi.E_RANGE and nb.value == need
        back = buf.download(np.zeros(need, np.uint8))
        assert (back == 0xA5).all()
        with pytest.raises(engine.BcfGpuError) as e:
            ctx.encode_bcf(o, n, IDS, cap_bytes=need - 1)
        assert e.value.code == abi.E_RANGE and e.value.needed == need
        rc = ctx.L.bcfgpu_mplp_encode_bcf(ctx.h, n, C.byref(o), ids, None, buf.ptr, need, off.ptr, C.byref(nb))
        assert rc == 0 and nb.value == need
        assert buf.download(np.zeros(need, np.uint8)).tobytes() == wdata.tobytes()
        np.testing.assert_array_equal(off.download(np.zeros(n + 1, np.uint64)), woff)


def test_planes_of_real_tiles_both_passes(golden_dir):
    """A small tile of the reference's fixtures through bcfgpu_mpileup, the SNP pass and the indel pass (the insertion at
    17:302 of mpileup.2.out): the blocks made from the planes in HBM are the numpy encoder's over the downloaded planes."""
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
            got = ctx.encode_bcf(o, t.n_sites, IDS, emit=emit)
            check_equal(got, want(fmt, IDS, res, emit))
            assert len(got[0]) > 20 * t.n_sites
            ctx.release(tb + list(ob.values()))
