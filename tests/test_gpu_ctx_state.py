"""A context's results do not depend on the calls made before: include/bcfgpu.h says which call ends what an earlier one left
in the context's workspace (the read pool, the SNP tile, the two indel tiles, the draw plan).  Every output kept across other
entry points must equal what the consumer gives right after its producer on a fresh context, byte for byte, and the oracle.
Orders the header rules out are refused (the pool a pileup was built from is gone) or run without the stale state (a draw plan
of a tile that has been rebuilt).  Caller-owned outputs are filled with a pattern first: only the parts the header calls valid
are compared."""
import ctypes as C

import numpy as np
import pytest

from bcftools_amd import abi, engine, host, synth
from bcftools_amd.lib import check
from tests.helpers import indeldrv, orc
from tests.test_gpu_parity import assert_mplp_equal, assert_call_equal

pytestmark = pytest.mark.gpu

FMT = abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD | abi.FMT_QS | abi.FMT_SCR | abi.INFO_SCR | abi.FMT_SP
PLANES = ("site", "pl", "dp4", "adf", "adr", "qs", "scr", "sp")


def _cfg(S, max_sites=20000, max_reads=1 << 21, **kw):
    return abi.default_cfg(S, max_sites=max_sites, max_reads=max_reads, fmt_flag=FMT, **kw)


def _same(a, b):
    for k in PLANES:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def _host(ctx, t):
    """A device tile's arrays as a HostTile."""
    S = ctx.cfg.n_smpl
    n, R = int(t.n_sites), int(t.n_reads)
    off, ref16 = np.zeros(n * S + 1, np.uint32), np.zeros(n, np.int8)
    rd, ep = np.zeros(R, np.uint32), np.zeros(R, np.uint8)
    aux = np.zeros(R, np.uint32) if t.is_indel else None
    for dst, src in ((off, t.plp_off), (ref16, t.ref16), (rd, t.rd), (ep, t.epos), (aux, t.aux)):
        if dst is not None and dst.nbytes:
            check(ctx.L.bcfgpu_memcpy_d2h(ctx.h, dst.ctypes.data, src, dst.nbytes))
    return host.HostTile(S, ref16, off, rd, ep, aux=aux, is_indel=int(t.is_indel))


def _mplp(ctx, t, fill=0):
    """bcfgpu_mpileup on a device tile, outputs filled with `fill` first."""
    o, ob, res = ctx.alloc_mplp_out(max(1, int(t.n_sites)))
    for b in ob.values():
        check(ctx.L.bcfgpu_memset(ctx.h, b.ptr, fill, b.nbytes))
    try:
        check(ctx.L.bcfgpu_mpileup(ctx.h, C.byref(t), C.byref(o)))
        ctx.sync()
        ctx._download(ob, res)
    finally:
        ctx.release(list(ob.values()))
    return res


def _gap_prep_tile(ctx, ref, cols, col_n):
    """bcfgpu_gap_prep_tile over columns `cols` of the last pileup (col_n: its entries per column), ZQ from the pool in HBM.
    Returns (dict: ret, aux = the tile's p->aux words, types, live_cols = the tile's columns; the tile)."""
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    E = int(col_n[cols].sum())
    out = dict(ret=np.zeros(len(cols), np.int32), aux=np.zeros(E, np.uint32), types=np.zeros((len(cols), 4), np.int32))
    par = abi.IndelIn()
    par.ref = ref
    for k, v in indeldrv.DEFAULTS.items():
        setattr(par, k, v)
    oo = abi.IndelOut()
    oo.ret, oo.p_aux, oo.indel_types = out["ret"].ctypes.data, out["aux"].ctypes.data, out["types"].ctypes.data
    t = abi.Tile()
    check(ctx.L.bcfgpu_gap_prep_tile(ctx.h, len(cols), cols.ctypes.data, None, C.byref(par), C.byref(oo), indeldrv.CAP, C.byref(t)))
    out["live_cols"] = np.ascontiguousarray(cols[out["ret"] == 0], dtype=np.int32)
    out["aux"] = out["aux"][:int(t.n_reads)].copy()
    return out, t


class Region:
    """One synthetic region with indel candidates (synth.indel_batch) on a context: bcfgpu_pileup, then on request the indel
    tile of bcfgpu_gap_prep_tile (all candidates, or a subset) and of bcfgpu_pileup_indel_tile (a subset)."""

    def __init__(self, ctx, seed, n_sites=12, n_smpl=6, depth=20.0, **kw):
        self.ctx = ctx
        self.b = synth.indel_batch(seed, n_sites, n_smpl, depth=depth, **kw)
        self.pool = indeldrv.DevicePool(ctx, self.b)          # bcfgpu_pileup over the whole reference
        self.snp = self.pool.tile

    def gtile(self, pick=None):
        """bcfgpu_gap_prep_tile over the candidate columns `pick` (indices into the batch's columns; None: all)."""
        p = self.pool
        return _gap_prep_tile(self.ctx, self.b["ref"], p.cols if pick is None else p.cols[pick], p.col_n)

    def itile(self, g, every=2):
        """bcfgpu_pileup_indel_tile over every `every`-th column of a gap_prep_tile result g (its p->aux words)."""
        ctx = self.ctx
        lc = g["live_cols"]
        n = self.pool.col_n[lc]
        beg = np.r_[0, np.cumsum(n)]
        sel = np.arange(0, len(lc), every)
        cols = np.ascontiguousarray(lc[sel], dtype=np.int32)
        aux = np.ascontiguousarray(np.concatenate([g["aux"][beg[i]:beg[i + 1]] for i in sel]) if len(sel) else np.zeros(0, np.uint32), dtype=np.uint32)
        t = abi.Tile()
        check(ctx.L.bcfgpu_pileup_indel_tile(ctx.h, len(cols), cols.ctypes.data, aux.ctypes.data, len(aux), C.byref(t)))
        assert int(t.n_reads) == len(aux)
        return t


# ---- the calls that may come between a producer and its consumer -------------------------------------------------------------
def _reads_struct(b):
    rd = abi.Reads()
    rd.n_reads = b["reads"]["n_reads"]
    for k in indeldrv.READ_KEYS:
        setattr(rd, k, b["reads"][k].ctypes.data)
    return rd


def step_baq(ctx, b):
    n, nb = int(b["reads"]["n_reads"]), len(b["reads"]["qual"])
    q, z, r = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8), np.zeros(n, np.int32)
    check(ctx.L.bcfgpu_baq(ctx.h, C.byref(_reads_struct(b)), b["ref"], len(b["ref"]), 3, q.ctypes.data, z.ctypes.data, r.ctypes.data))


def step_cap_mapq(ctx, b):
    cap = np.zeros(int(b["reads"]["n_reads"]), np.int32)
    check(ctx.L.bcfgpu_cap_mapq(ctx.h, C.byref(_reads_struct(b)), b["ref"], len(b["ref"]), 50, cap.ctypes.data))


def step_overlap(ctx, b):
    n = int(b["reads"]["n_reads"])
    pa, pb = np.arange(0, n - 1, 2, dtype=np.int32)[:64], np.arange(1, n, 2, dtype=np.int32)[:64]
    q = np.zeros(len(b["reads"]["qual"]), np.uint8)
    check(ctx.L.bcfgpu_overlap_tweak(ctx.h, C.byref(_reads_struct(b)), len(pa), pa.ctypes.data, pb.ctypes.data, q.ctypes.data))


def step_gap_prep(ctx, b):
    indeldrv.gap_prep_gpu(ctx, b)


def _call_input(seed, S, n_sites=24):
    tile = synth.numpy_tile(seed, n_sites, S, depth=15.0, var_rate=0.4)
    cfg = _cfg(S)
    m = orc.mpileup(cfg, tile)
    cin = host.CallInput(S, m.site["n_alleles"], np.maximum(m.site["unseen"], 0), m.pl.astype(np.int32), m.site["qsum"],
                         i16=m.site["anno"].astype(np.float32))
    return tile, m, cin


def step_mcall(ctx, b):
    _, _, cin = _call_input(5, ctx.cfg.n_smpl)
    ctx.mcall(cin)


def step_gvcf(ctx, b):
    tile, m, _ = _call_input(6, ctx.cfg.n_smpl)
    ctx.gvcf_blocks(m, np.arange(tile.n_sites, dtype=np.int32), [1, 5, 10])


def _compact(ctx, cin):
    """bcfgpu_mcall into device planes, then both forms of bcfgpu_compact_calls over them, each into a buffer of its own.
    Returns (the calls, records of the blocking form, their count, records of the queued form, their count)."""
    d = abi.CallIn()
    d.n_sites, d.n_gt_max, d.n_al_max = cin.n_sites, cin.n_gt_max, cin.n_al_max
    keep = []
    for k in ("nals", "unseen", "pl", "qs", "i16"):
        keep.append(ctx.to_device(getattr(cin, k)))
        setattr(d, k, keep[-1].ptr)
    co, cb, cres = ctx.alloc_call_out(cin.n_sites, cin.n_gt_max)
    for b in cb.values():
        check(ctx.L.bcfgpu_memset(ctx.h, b.ptr, 0, b.nbytes))
    cap = 4 << 20
    buf, buf2, cnt = ctx.buf(cap), ctx.buf(cap), ctx.buf(64)
    nb, nr, nb2, nr2 = C.c_uint64(), C.c_uint32(), C.c_uint64(), C.c_uint32()
    try:
        check(ctx.L.bcfgpu_mcall(ctx.h, C.byref(d), C.byref(co)))
        check(ctx.L.bcfgpu_compact_calls(ctx.h, cin.n_sites, 0, None, C.byref(co), cin.n_gt_max, 0, buf.ptr, cap, C.byref(nb), C.byref(nr)))
        check(ctx.L.bcfgpu_compact_calls_async(ctx.h, cin.n_sites, 0, None, C.byref(co), cin.n_gt_max, 0, buf2.ptr, cap, cnt.ptr))
        check(ctx.L.bcfgpu_compact_counts(ctx.h, cnt.ptr, C.byref(nb2), C.byref(nr2)))
        ctx.sync()
        ctx._download(cb, cres)
        recs, recs2 = np.zeros(int(nb.value), np.uint8), np.zeros(int(nb2.value), np.uint8)
        for a, bb in ((recs, buf), (recs2, buf2)):
            if a.nbytes:
                check(ctx.L.bcfgpu_memcpy_d2h(ctx.h, a.ctypes.data, bb.ptr, a.nbytes))
    finally:
        ctx.release(keep + list(cb.values()) + [buf, buf2, cnt])
    return cres, recs, int(nr.value), recs2, int(nr2.value)


def step_compact(ctx, b):
    _, recs, nr, recs2, nr2 = _compact(ctx, _call_input(7, ctx.cfg.n_smpl)[2])
    assert nr == nr2 > 0 and recs.tobytes() == recs2.tobytes()


def step_entries(ctx, reg):
    p = reg.pool
    cap = int(p.col_n[p.cols].sum())
    so = np.zeros(len(p.cols) * ctx.cfg.n_smpl + 1, np.int32)
    pr, pq, pi = (np.zeros(cap, np.int32) for _ in range(3))
    check(ctx.L.bcfgpu_pileup_entries(ctx.h, len(p.cols), p.cols.ctypes.data, so.ctypes.data, pr.ctypes.data, pq.ctypes.data, pi.ctypes.data, cap))


def step_pool_upload(ctx, seed):
    """A different region's reads replace the context's pool."""
    b = synth.indel_batch(seed, 4, ctx.cfg.n_smpl, depth=10.0)
    reads, mapq, _, _ = synth.indel_pool(b)
    rd = abi.Reads()
    rd.n_reads = reads["n_reads"]
    for k in indeldrv.READ_KEYS:
        setattr(rd, k, reads[k].ctypes.data)
    check(ctx.L.bcfgpu_pool_upload(ctx.h, C.byref(rd), None, mapq.ctypes.data))


def host_steps(ctx, b):
    """The host-pointer stages and the call-side entries: they read nothing a pileup, a pool or a plan left."""
    for f in (step_baq, step_cap_mapq, step_overlap, step_mcall, step_gvcf, step_compact):
        f(ctx, b)


# ---- a. kept outputs survive every call the header lets come between -----------------------------------------------------------
@pytest.fixture(scope="module")
def fresh():
    """Each consumer right after its producer on a fresh context (and the oracle on the tile it ran on)."""
    S, out = 6, {}
    with engine.Context(_cfg(S)) as ctx:
        reg = Region(ctx, 101)
        out["snp_tile"] = _host(ctx, reg.snp)
        out["snp"] = _mplp(ctx, reg.snp)
    with engine.Context(_cfg(S)) as ctx:
        reg = Region(ctx, 101)
        g, gt = reg.gtile()
        out["g"], out["gt_tile"], out["gt"] = g, _host(ctx, gt), _mplp(ctx, gt)
    with engine.Context(_cfg(S)) as ctx:
        reg = Region(ctx, 101)
        g, _ = reg.gtile()
        it = reg.itile(g)
        out["it_tile"], out["it"] = _host(ctx, it), _mplp(ctx, it)
    cfg = _cfg(S)
    for k in ("snp", "gt", "it"):
        assert_mplp_equal(out[k], orc.mpileup(cfg, out[k + "_tile"]))
    assert out["gt_tile"].n_sites > 2 and out["it_tile"].n_sites >= 1 and out["it_tile"].n_sites < out["gt_tile"].n_sites
    return out


def test_snp_tile_survives_the_calls_between(fresh):
    with engine.Context(_cfg(6)) as ctx:
        reg = Region(ctx, 101)
        host_steps(ctx, reg.b)
        step_gap_prep(ctx, reg.b)
        step_entries(ctx, reg)
        g, _ = reg.gtile(np.arange(0, len(reg.pool.cols), 2))
        reg.itile(g, every=1)
        step_pool_upload(ctx, 55)                                 # the tile needs no pool
        _same(_mplp(ctx, reg.snp), fresh["snp"])


def test_gap_prep_tile_survives_the_calls_between(fresh):
    """bcfgpu_pileup_indel_tile in between: before the two calls had slots of their own, it overwrote this tile's records."""
    with engine.Context(_cfg(6)) as ctx:
        reg = Region(ctx, 101)
        g, gt = reg.gtile()
        assert g["aux"].tobytes() == fresh["g"]["aux"].tobytes()
        host_steps(ctx, reg.b)
        step_entries(ctx, reg)
        reg.itile(g, every=3)
        step_pool_upload(ctx, 56)
        _same(_mplp(ctx, gt), fresh["gt"])


def test_indel_tile_survives_the_calls_between(fresh):
    """bcfgpu_gap_prep_tile in between: before the two calls had slots of their own, it overwrote this tile."""
    with engine.Context(_cfg(6)) as ctx:
        reg = Region(ctx, 101)
        g, _ = reg.gtile()
        it = reg.itile(g)
        host_steps(ctx, reg.b)
        step_gap_prep(ctx, reg.b)
        step_entries(ctx, reg)
        reg.gtile(np.arange(1, len(reg.pool.cols), 2))
        step_pool_upload(ctx, 57)
        _same(_mplp(ctx, it), fresh["it"])


def _pool_chain(ctx, b):
    reads, mapq, smpl, _ = synth.indel_pool(b)
    rd = abi.Reads()
    rd.n_reads = reads["n_reads"]
    for k in indeldrv.READ_KEYS:
        setattr(rd, k, reads[k].ctypes.data)
    n = int(reads["n_reads"])
    check(ctx.L.bcfgpu_pool_upload(ctx.h, C.byref(rd), None, mapq.ctypes.data))
    check(ctx.L.bcfgpu_pool_baq(ctx.h, b["ref"], len(b["ref"]), 3, None))
    cap = np.zeros(n, np.int32)
    check(ctx.L.bcfgpu_pool_cap_mapq(ctx.h, b["ref"], len(b["ref"]), 50, cap.ctypes.data))
    keep = (cap >= 0).astype(np.uint8)
    keep[::13] = 0
    check(ctx.L.bcfgpu_pool_keep(ctx.h, keep.ctypes.data))
    pa, pb = np.arange(0, n - 1, 2, dtype=np.int32)[:32], np.arange(1, n, 2, dtype=np.int32)[:32]
    check(ctx.L.bcfgpu_pool_overlap_tweak(ctx.h, len(pa), pa.ctypes.data, pb.ctypes.data))
    return reads, smpl


def _pool_download(ctx, reads):
    nb, n = len(reads["qual"]), int(reads["n_reads"])
    q, z, m = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8), np.zeros(n, np.uint8)
    check(ctx.L.bcfgpu_pool_download(ctx.h, q.ctypes.data, z.ctypes.data, m.ctypes.data))
    return q, z, m


def _pool_pileup(ctx, b, smpl):
    t = abi.Tile()
    L = len(b["ref"])
    col_n = np.zeros(L, np.int32)
    check(ctx.L.bcfgpu_pool_pileup(ctx.h, smpl.ctypes.data, None, 0, L, b["ref"], L, C.byref(t), col_n.ctypes.data, None))
    return t, col_n


def test_pool_and_its_tile_survive_the_calls_between():
    """The pool after the whole chain of pool stages, read back and piled up after the host-pointer stages; then the tile of
    bcfgpu_pool_pileup, run after those stages, bcfgpu_gap_prep_tile, bcfgpu_pileup_entries and a new pool."""
    b = synth.indel_batch(102, 10, 6, depth=20.0)
    cols = np.ascontiguousarray(b["pos"], dtype=np.int32)
    with engine.Context(_cfg(6)) as ctx:
        reads, smpl = _pool_chain(ctx, b)
        want = _pool_download(ctx, reads)
        t, _ = _pool_pileup(ctx, b, smpl)
        want_tile, want_res = _host(ctx, t), _mplp(ctx, t)
    assert_mplp_equal(want_res, orc.mpileup(_cfg(6), want_tile))
    with engine.Context(_cfg(6)) as ctx:
        reads, smpl = _pool_chain(ctx, b)
        host_steps(ctx, b)
        step_gap_prep(ctx, b)
        got = _pool_download(ctx, reads)
        t, col_n = _pool_pileup(ctx, b, smpl)
        host_steps(ctx, b)
        g, _ = _gap_prep_tile(ctx, b["ref"], cols, col_n)
        assert len(g["live_cols"]) > 0
        so = np.zeros(len(cols) * 6 + 1, np.int32)
        e = np.zeros(int(col_n[cols].sum()), np.int32)
        check(ctx.L.bcfgpu_pileup_entries(ctx.h, len(cols), cols.ctypes.data, so.ctypes.data, e.ctypes.data, e.ctypes.data, e.ctypes.data, len(e)))
        step_pool_upload(ctx, 59)
        got_tile, got_res = _host(ctx, t), _mplp(ctx, t)
    for x, y in zip(got, want):
        assert x.tobytes() == y.tobytes()
    for k in ("plp_off", "ref16", "rd", "epos"):
        assert getattr(got_tile, k).tobytes() == getattr(want_tile, k).tobytes(), k
    _same(got_res, want_res)


def _deep_tile(seed, S=4, n_sites=6):
    rng = np.random.default_rng(seed)
    d = rng.poisson(30, n_sites * S)
    d[[1, 6, 13, 22]] = rng.integers(300, 700, 4)
    R = int(d.sum())
    rd = (rng.choice([11, 25, 37, 40], R) | (60 << 8) | ((1 << rng.integers(0, 4, R)) << 16) | (rng.integers(0, 2, R) << 20)
          | (rng.integers(0, 40, R) << 24)).astype(np.uint32)
    return host.HostTile(S, rng.choice([1, 2, 4, 8], n_sites).astype(np.int8), np.r_[0, np.cumsum(d)].astype(np.uint32), rd,
                         rng.integers(0, 100, R).astype(np.uint8))


def test_draw_plan_survives_the_calls_between():
    """errmod_plan on a caller's tile, then everything that is no mpileup / pipeline of the SNP pass, then the tile's mpileup:
    errmod_cal's own draw from a fresh generator (the oracle's rule 0), as when the mpileup follows the plan at once."""
    deep = _deep_tile(8)
    want = orc.mpileup(_cfg(4), deep, deep_rule=0)
    got = []
    for between in (False, True):
        with engine.Context(_cfg(4)) as ctx:
            dt, tb = ctx.upload_tile(deep)
            check(ctx.L.bcfgpu_errmod_plan(ctx.h, C.byref(dt), None, None, None))
            if between:
                reg = Region(ctx, 103, n_smpl=4)                  # a pileup of its own: another SNP tile, not this one
                host_steps(ctx, reg.b)
                step_gap_prep(ctx, reg.b)
                step_entries(ctx, reg)
                g, _ = reg.gtile()
                reg.itile(g)
            got.append(_mplp(ctx, dt))
            n = C.c_uint32()
            check(ctx.L.bcfgpu_truncated_cells(ctx.h, C.byref(n)))
            assert n.value == 0
            ctx.release(tb)
    assert_mplp_equal(got[1], want)
    _same(got[1], got[0])


# ---- b. orders outside the header's rules are refused or run without the stale state ---------------------------------------
def test_calls_on_a_replaced_pool_are_refused():
    with engine.Context(_cfg(6)) as ctx:
        reg = Region(ctx, 104)
        step_pool_upload(ctx, 58)
        p = reg.pool
        so = np.zeros(len(p.cols) * 6 + 1, np.int32)
        cap = int(p.col_n[p.cols].sum())
        arr = np.zeros(cap, np.int32)
        assert ctx.L.bcfgpu_pileup_entries(ctx.h, len(p.cols), p.cols.ctypes.data, so.ctypes.data, arr.ctypes.data, arr.ctypes.data,
                                           arr.ctypes.data, cap) == abi.E_ARG
        assert b"gone" in ctx.L.bcfgpu_last_error()
        aux = np.zeros(cap, np.uint32)
        t = abi.Tile()
        assert ctx.L.bcfgpu_pileup_indel_tile(ctx.h, len(p.cols), p.cols.ctypes.data, aux.ctypes.data, cap, C.byref(t)) == abi.E_ARG
        with pytest.raises(engine.BcfGpuError) as e:
            reg.gtile()
        assert e.value.code == abi.E_ARG and "gone" in str(e.value)
        _same(_mplp(ctx, reg.snp), _mplp_fresh_snp(104))           # the tile itself stays valid


def _mplp_fresh_snp(seed):
    with engine.Context(_cfg(6)) as ctx:
        return _mplp(ctx, Region(ctx, seed).snp)


def _deep_cells(tile, min_baseQ=13):
    """Cells of more than 255 usable reads (the ones errmod_cal draws for)."""
    w = tile.rd
    ok = (w & abi.RD_SKIP) == 0
    if not tile.is_indel:
        ok &= ((w & abi.RD_DEL) == 0) & ((w & 0xff) >= min_baseQ)
    c = np.r_[0, np.cumsum(ok, dtype=np.int64)]
    off = tile.plp_off.astype(np.int64)
    return int(((c[off[1:]] - c[off[:-1]]) > abi.MAX_DEPTH).sum())


def test_a_plan_does_not_follow_its_tile_into_a_rebuilt_one():
    """errmod_plan on the pileup's tile A, then a new pileup whose records start where A's did (the slot was grown beforehand by
    a larger pileup): B with more reads than A, and A itself again -- the same reads, so only the rebuild dropping the plan keeps
    it from being taken.  Each runs without A's plan (the first 255 usable reads of a deep cell), as on a fresh context."""
    S = 3
    rng = np.random.default_rng(9)
    L = 400
    ref = bytes(rng.choice(list(b"ACGT"), L).astype(np.uint8))
    from tests.helpers import ovlfuzz, mplpdrv as M

    def pool(n_per, lo=0, hi=30):
        flat = []
        for s in range(S):
            rl = sorted((ovlfuzz.make_read(rng, int(rng.integers(lo, hi)), 80) for _ in range(n_per)), key=lambda r: r.pos)
            for r in rl:
                r.mapq, r.flag = 60, 0
            flat += rl
        rd, d = M.pack_reads(flat)
        return rd, d, np.full(len(flat), 60, np.uint8), np.repeat(np.arange(S, dtype=np.int32), n_per)

    def pileup(ctx, P):
        rd, d, mapq, smpl = P
        t = abi.Tile()
        check(ctx.L.bcfgpu_pileup(ctx.h, C.byref(rd), mapq.ctypes.data, smpl.ctypes.data, 0, 120, ref, L, C.byref(t), None, None))
        return t

    def plan(ctx, t):
        check(ctx.L.bcfgpu_errmod_plan(ctx.h, C.byref(t), None, None, None))
    big, A, B = pool(900), pool(400), pool(700)
    want = {}
    for name, P in (("A", A), ("B", B)):
        with engine.Context(_cfg(S)) as ctx:
            t = pileup(ctx, P)
            want[name], host_t = _mplp(ctx, t), _host(ctx, t)
        assert _deep_cells(host_t) > 0
        assert_mplp_equal(want[name], orc.mpileup(_cfg(S), host_t, deep_rule=1))
    with engine.Context(_cfg(S)) as ctx:                          # with A's plan taken, A's likelihoods differ: the case is real
        ta = pileup(ctx, A)
        plan(ctx, ta)
        assert _mplp(ctx, ta).pl.tobytes() != want["A"].pl.tobytes()
    with engine.Context(_cfg(S)) as ctx:
        pileup(ctx, big)
        ta = pileup(ctx, A)
        plan(ctx, ta)
        tb = pileup(ctx, B)
        assert tb.rd == ta.rd and int(tb.n_reads) > int(ta.n_reads)
        _same(_mplp(ctx, tb), want["B"])
        ta = pileup(ctx, A)
        plan(ctx, ta)
        ta2 = pileup(ctx, A)
        assert ta2.rd == ta.rd and ta2.n_reads == ta.n_reads
        _same(_mplp(ctx, ta2), want["A"])


def test_an_indel_plan_survives_the_other_indel_tile():
    """errmod_plan on the indel tile of bcfgpu_gap_prep_tile, then bcfgpu_pileup_indel_tile (a tile of its own) and
    bcfgpu_pileup_entries, then the planned tile's mpileup: errmod_cal's own draw (the oracle's rule 0), as right after the plan.
    The plan is seen to be taken by bcfgpu_truncated_cells, which counts the deep cells of a launch without one."""
    S = 2
    got, cut = [], []
    for mode in ("plan", "plan, then the other calls", "no plan"):
        with engine.Context(_cfg(S)) as ctx:
            reg = Region(ctx, 113, n_sites=3, n_smpl=S, depth=320.0, max_depth=450)
            g, gt = reg.gtile()
            assert len(g["live_cols"]) > 0
            if mode != "no plan":
                check(ctx.L.bcfgpu_errmod_plan(ctx.h, None, C.byref(gt), g["live_cols"].ctypes.data, None))
            if mode == "plan, then the other calls":
                reg.itile(g, every=1)
                step_entries(ctx, reg)
            got.append((_host(ctx, gt), _mplp(ctx, gt)))
            n = C.c_uint32()
            check(ctx.L.bcfgpu_truncated_cells(ctx.h, C.byref(n)))
            cut.append(n.value)
    tile = got[0][0]
    assert cut == [0, 0, _deep_cells(tile)] and cut[2] > 0
    assert_mplp_equal(got[0][1], orc.mpileup(_cfg(S), tile, deep_rule=0))
    assert got[1][0].rd.tobytes() == tile.rd.tobytes() and got[1][0].aux.tobytes() == tile.aux.tobytes()
    _same(got[1][1], got[0][1])


def _region_results(ctx, seed, n_sites, depth):
    reg = Region(ctx, seed, n_sites=n_sites, depth=depth)
    g, gt = reg.gtile()
    return [(_host(ctx, reg.snp), _mplp(ctx, reg.snp)), (_host(ctx, gt), _mplp(ctx, gt))]


def _pipeline_alone(cfg, tile, ploidy=None, grp=None, plan=False):
    with engine.Context(cfg) as ctx:
        return _pipeline(ctx, tile, ploidy, grp, plan)


def _pipeline(ctx, tile, ploidy=None, grp=None, plan=False):
    if not plan:
        return ctx.pipeline(tile, ploidy=ploidy, grp=grp)
    dt, tb = ctx.upload_tile(tile)
    try:
        check(ctx.L.bcfgpu_errmod_plan(ctx.h, C.byref(dt), None, None, None))
        mo, mb, mres = ctx.alloc_mplp_out(tile.n_sites)
        co, cb, cres = ctx.alloc_call_out(tile.n_sites, abi.MAX_PL)
        for b in list(mb.values()) + list(cb.values()):
            check(ctx.L.bcfgpu_memset(ctx.h, b.ptr, 0, b.nbytes))
        check(ctx.L.bcfgpu_pipeline(ctx.h, C.byref(dt), None, None, C.byref(mo), C.byref(co)))
        ctx.sync()
        ctx._download(mb, mres)
        ctx._download(cb, cres)
        ctx.release(list(mb.values()) + list(cb.values()))
    finally:
        ctx.release(tb)
    return mres, cres


def _call_want(cfg, m, ploidy=None, grp=None):
    ad = None
    if grp is not None:                                          # as tests/test_gpu_parity.py forms FORMAT/AD
        na = m.site["n_alleles"]
        ad = np.where(np.arange(5)[None, :, None] < na[:, None, None], m.adf.astype(np.int32) + m.adr.astype(np.int32),
                      abi.INT32_VECTOR_END).astype(np.int32)
    cin = host.CallInput(cfg.n_smpl, m.site["n_alleles"], np.maximum(m.site["unseen"], 0), m.pl.astype(np.int32), m.site["qsum"],
                         ploidy=ploidy, grp=grp, ad=ad, i16=m.site["anno"].astype(np.float32))
    return orc.mcall(cfg, cin)


def _same_call(a, b):
    for k in ("site", "gt", "pl", "gq", "gp"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def _pool_region(ctx, b):
    """One region as host/bcfgpu_sam.c runs it per tile: the pool chain, bcfgpu_pool_pileup, bcfgpu_gap_prep_tile on the
    candidates (ZQ from bcfgpu_pool_baq's copy in HBM), bcfgpu_errmod_plan_visit over both passes, the mpileup of each tile."""
    reads, smpl = _pool_chain(ctx, b)
    t, col_n = _pool_pileup(ctx, b, smpl)
    g, gt = _gap_prep_tile(ctx, b["ref"], b["pos"], col_n)
    assert len(g["live_cols"]) > 0
    visit = np.ones(int(t.n_sites), np.uint8)
    visit[::7] = 0
    visit[g["live_cols"]] = 1
    check(ctx.L.bcfgpu_errmod_plan_visit(ctx.h, C.byref(t), visit.ctypes.data, C.byref(gt), g["live_cols"].ctypes.data, None))
    return g, [(_host(ctx, t), _mplp(ctx, t)), (_host(ctx, gt), _mplp(ctx, gt))]


def test_a_region_after_a_larger_one_is_what_it_is_alone():
    """The pool chain of a region i with more sites, reads and candidates, then of a smaller and shallower region i+1 on the same
    context (the C driver's tile loop): every stage output, tile and result as on a fresh context, and the oracle's."""
    S = 6
    regions = [synth.indel_batch(105, 24, S, depth=30.0), synth.indel_batch(106, 6, S, depth=8.0)]
    with engine.Context(_cfg(S)) as ctx:
        seq = [_pool_region(ctx, b) for b in regions]
    for b, (g, got) in zip(regions, seq):
        with engine.Context(_cfg(S)) as ctx:
            ga, alone = _pool_region(ctx, b)
        for k in ("ret", "aux", "types"):
            assert g[k].tobytes() == ga[k].tobytes(), k
        for (tile, res), (at, ares) in zip(got, alone):
            for k in ("plp_off", "rd", "epos", "aux"):
                assert (getattr(tile, k) is None) == (getattr(at, k) is None)
                if getattr(tile, k) is not None:
                    assert getattr(tile, k).tobytes() == getattr(at, k).tobytes(), k
            _same(res, ares)
            assert _deep_cells(tile) == 0                         # (the plan draws nothing: rule 1 is the oracle's answer)
            assert_mplp_equal(res, orc.mpileup(_cfg(S), tile))


def test_snp_and_indel_work_alternating_with_and_without_a_plan():
    """Deep SNP tiles through bcfgpu_pipeline with an errmod plan and without, between indel tiles of a region, deepest first."""
    S = 4
    cfg = _cfg(S)
    deep, shallow = _deep_tile(11, S, 8), synth.numpy_tile(12, 10, S, depth=12.0, var_rate=0.3)
    with engine.Context(cfg) as ctx:
        seq = [_pipeline(ctx, deep, plan=True)]
        reg = Region(ctx, 107, n_smpl=S)
        g, gt = reg.gtile()
        gres = _mplp(ctx, gt)
        seq.append(_pipeline(ctx, deep, plan=False))
        it = reg.itile(g)
        ires = _mplp(ctx, it)
        seq.append(_pipeline(ctx, shallow, plan=True))
        seq.append(_pipeline(ctx, shallow, plan=False))
    wants = [(deep, True, 0), (deep, False, 1), (shallow, True, 0), (shallow, False, 1)]
    for (m, c), (t, plan, rule) in zip(seq, wants):
        am, ac = _pipeline_alone(cfg, t, plan=plan)
        _same(m, am)
        _same_call(c, ac)
        mw = orc.mpileup(cfg, t, deep_rule=rule)
        assert_mplp_equal(m, mw)
        assert_call_equal(c, _call_want(cfg, mw), S)
    with engine.Context(cfg) as ctx:
        reg = Region(ctx, 107, n_smpl=S)
        g, gt = reg.gtile()
        _same(gres, _mplp(ctx, gt))
        _same(ires, _mplp(ctx, reg.itile(g)))


def test_groups_and_ploidy_large_tile_then_small():
    """call -G with a ploidy array: the groups' workspace only grows; a small tile after a large one calls as it does alone."""
    S, n_grp = 40, 3
    cfg = abi.default_cfg(S, max_sites=256, max_reads=1 << 21, fmt_flag=FMT | abi.FMT_AD, n_grp=n_grp)
    rng = np.random.default_rng(13)
    grp = rng.integers(0, n_grp, S).astype(np.int32)
    ploidy = rng.choice([1, 2, 2], S).astype(np.uint8)
    big, small = synth.numpy_tile(14, 256, S, depth=6.0, var_rate=0.3), synth.numpy_tile(15, 16, S, depth=6.0, var_rate=0.5)
    with engine.Context(cfg) as ctx:
        seq = [ctx.pipeline(big, ploidy=ploidy, grp=grp), ctx.pipeline(small, ploidy=ploidy, grp=grp)]
    for (m, c), t in zip(seq, (big, small)):
        am, ac = _pipeline_alone(cfg, t, ploidy, grp)
        _same(m, am)
        _same_call(c, ac)
        mw = orc.mpileup(cfg, t)
        assert_mplp_equal(m, mw)
        assert_call_equal(c, _call_want(cfg, mw, ploidy, grp), S)


def test_gvcf_and_compact_large_then_small():
    """bcfgpu_gvcf_blocks and both forms of bcfgpu_compact_calls over a 300-site call set, then over a 20-site one, on one
    context: each gives what a fresh context gives it alone, byte for byte; the blocks are the oracle's gvcf_write, the calls
    the oracle's mcall, the records one per call with ret >= 0."""
    S = 5
    sets = [_call_input(seed, S, n) for seed, n in ((16, 300), (17, 20))]

    def run(ctx, tile, m, cin):
        return ctx.gvcf_blocks(m, np.arange(tile.n_sites, dtype=np.int32), [1, 5, 10]), _compact(ctx, cin)
    with engine.Context(_cfg(S)) as ctx:
        seq = [run(ctx, *x) for x in sets]
    for (tile, m, cin), (g, (cres, recs, nr, recs2, nr2)) in zip(sets, seq):
        with engine.Context(_cfg(S)) as ctx:
            ga, (cres_a, recs_a, nr_a, _, _) = run(ctx, tile, m, cin)
        nb = g.n_blocks
        assert nb == ga.n_blocks
        for k in ("blk", "min_dp"):
            assert getattr(g, k).tobytes() == getattr(ga, k).tobytes(), k
        for k in ("block", "dp", "pl"):
            assert getattr(g, k)[:nb].tobytes() == getattr(ga, k)[:nb].tobytes(), k
        w = orc.gvcf_blocks(m, np.arange(tile.n_sites, dtype=np.int32), [1, 5, 10])
        assert nb == w.n_blocks > 0
        for k in ("blk", "min_dp"):
            np.testing.assert_array_equal(getattr(g, k), getattr(w, k))
        np.testing.assert_array_equal(g.dp[:nb], w.dp[:nb])
        np.testing.assert_array_equal(g.pl[:nb].astype(np.int32), w.pl[:nb])
        _same_call(cres, cres_a)
        cw = orc.mcall(_cfg(S), cin)
        assert_call_equal(cres, cw, S)
        assert nr == nr_a == nr2 == int((cw.site["ret"] >= 0).sum()) > 0
        assert recs.tobytes() == recs_a.tobytes() == recs2.tobytes() and len(recs) > 0


# ---- d. caller-owned outputs: only what the header calls valid is written ---------------------------------------------------
def _mask_mplp(r):
    """Zero everything the header leaves undefined: PL planes past n_alleles*(n_alleles+1)/2, AD/QS planes past n_alleles."""
    na = r.site["n_alleles"].astype(np.int64)
    for i in range(r.n_sites):
        r.pl[i, na[i] * (na[i] + 1) // 2:] = 0
        for k in ("adf", "adr", "qs"):
            getattr(r, k)[i, na[i]:] = 0
    return r


def test_outputs_are_written_where_the_header_says_they_are_valid():
    S = 30
    cfg = _cfg(S, max_sites=64)
    tile = synth.numpy_tile(18, 64, S, depth=20.0, var_rate=0.4, ref_n_rate=0.05)
    mw = orc.mpileup(cfg, tile)
    cw = _call_want(cfg, mw)
    with engine.Context(cfg) as ctx:
        dt, tb = ctx.upload_tile(tile)
        got = _mplp(ctx, dt, fill=0xA5)
        assert_mplp_equal(_mask_mplp(got), _mask_mplp(orc.mpileup(cfg, tile)))
        cin = host.CallInput(S, mw.site["n_alleles"], np.maximum(mw.site["unseen"], 0), mw.pl.astype(np.int32), mw.site["qsum"],
                             i16=mw.site["anno"].astype(np.float32))
        d = abi.CallIn()
        d.n_sites, d.n_gt_max, d.n_al_max = cin.n_sites, cin.n_gt_max, cin.n_al_max
        keep = []
        for k in ("nals", "unseen", "pl", "qs", "i16"):
            keep.append(ctx.to_device(getattr(cin, k)))
            setattr(d, k, keep[-1].ptr)
        co, cb, cres = ctx.alloc_call_out(cin.n_sites, cin.n_gt_max)
        for b in cb.values():
            check(ctx.L.bcfgpu_memset(ctx.h, b.ptr, 0xA5, b.nbytes))
        check(ctx.L.bcfgpu_mcall(ctx.h, C.byref(d), C.byref(co)))
        ctx.sync()
        ctx._download(cb, cres)
        assert_call_equal(cres, cw, S)
        # the fused pipeline: its call outputs and mpileup planes
        mo, mb, mres = ctx.alloc_mplp_out(tile.n_sites)
        co2, cb2, cres2 = ctx.alloc_call_out(tile.n_sites, abi.MAX_PL)
        for b in list(mb.values()) + list(cb2.values()):
            check(ctx.L.bcfgpu_memset(ctx.h, b.ptr, 0xA5, b.nbytes))
        check(ctx.L.bcfgpu_pipeline(ctx.h, C.byref(dt), None, None, C.byref(mo), C.byref(co2)))
        ctx.sync()
        ctx._download(mb, mres)
        ctx._download(cb2, cres2)
        assert_mplp_equal(_mask_mplp(mres), _mask_mplp(orc.mpileup(cfg, tile)))
        assert_call_equal(cres2, _call_want(cfg, mw), S)
        ctx.release(tb + keep)


# ---- e. two contexts on one device, their calls interleaved ----------------------------------------------------------------
def test_two_contexts_interleaved():
    S = 6
    alone = []
    for seed in (108, 109):
        with engine.Context(_cfg(S)) as ctx:
            alone.append(_region_results(ctx, seed, 8, 15.0))
    with engine.Context(_cfg(S)) as c1, engine.Context(_cfg(S)) as c2:
        r1, r2 = Region(c1, 108, n_sites=8, depth=15.0), Region(c2, 109, n_sites=8, depth=15.0)
        g1, t1 = r1.gtile()
        g2, t2 = r2.gtile()
        got = [[None, None], [None, None]]
        got[1][0] = (_host(c2, r2.snp), _mplp(c2, r2.snp))
        got[0][1] = (_host(c1, t1), _mplp(c1, t1))
        got[0][0] = (_host(c1, r1.snp), _mplp(c1, r1.snp))
        got[1][1] = (_host(c2, t2), _mplp(c2, t2))
    for g, a in zip(got, alone):
        for (gt_tile, gres), (at, ares) in zip(g, a):
            assert gt_tile.rd.tobytes() == at.rd.tobytes() and gt_tile.plp_off.tobytes() == at.plp_off.tobytes()
            _same(gres, ares)
