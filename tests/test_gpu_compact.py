"""bcfgpu_compact_calls[_async] (bcftools_amd/csrc/gather.hip) against the plain packer of tests/helpers/callrec.py, byte for
byte, into buffers that were NOT zeroed first:

  A. on call planes the test makes itself (the compaction reads nothing else): every variants_only mode, 255 / 256 / 257 sites
     around the size kernel's grid, every value of 2S mod 4, a NULL site-record array, a plane stride that is not MAX_PL,
     a tile that compacts to nothing, no sites at all;
  B. the capacity contract: a buffer too small is not touched and the size comes back, in both forms; cap_bytes = 0 asks;
  C. the records and the call records of bcfgpu_mcall and of bcfgpu_pipeline do not depend on what their output buffers held;
  D. bcfgpu_gather_bytes over a communicator of one rank.
"""
import ctypes as C

import numpy as np
import pytest

from bcftools_amd import abi, host, synth
from bcftools_amd.lib import check
from tests.helpers import callrec, orc
from tests.test_call_records import synthetic_calls, assert_case_is_telling
from tests.test_gpu_mcall_random import random_records
from tests.test_gpu_parity import assert_call_equal

pytestmark = pytest.mark.gpu

FILL, SITE0, SLACK = 0xA5, 70001, 64
SHAPES = [(1, 1), (255, 2), (256, 3), (257, 65), (513, 130), (40, 64)]


class Planes:
    """Synthetic call planes of one shape in HBM, and their host copies."""

    def __init__(self, ctx, seed, n_sites, n_smpl, n_gt_planes, pin=None):
        self.ctx, self.n_sites, self.n_smpl, self.n_gt_planes = ctx, n_sites, n_smpl, n_gt_planes
        self.cs, self.gt, self.pl, self.ms = synthetic_calls(seed, n_sites, n_smpl, n_gt_planes)
        if pin is not None:
            pin(self.cs)
        self.bufs = [ctx.to_device(a if a.nbytes else np.zeros(16, np.uint8)) for a in (self.cs, self.gt, self.pl, self.ms)]
        self.co = abi.CallOut()
        self.co.site, self.co.gt, self.co.pl = (b.ptr for b in self.bufs[:3])
        self.d_ms = self.bufs[3].ptr

    def want(self, mode, with_ms=True):
        return callrec.pack(self.cs, self.gt, self.pl, self.n_smpl, self.n_gt_planes, SITE0, mode, self.ms if with_ms else None)

    def free(self):
        self.ctx.release(self.bufs)


def run_compact(ctx, n_sites, co, d_ms, n_gt_planes, mode, cap, alloc, queued, site0=SITE0, null_buf=False):
    """One compaction into a buffer of `alloc` bytes pre-filled with FILL, of which the call is told `cap`.  Returns (return
    code, n_bytes, n_rec, the whole buffer afterwards, the four counters of the queued form or None)."""
    buf = ctx.to_device(np.full(max(alloc, 16), FILL, np.uint8))
    cnt = ctx.to_device(np.full(4, 0x5A5A5A5A5A5A5A5A, np.uint64))
    nb, nr = C.c_uint64(12345), C.c_uint32(12345)
    counts = None
    try:
        d_buf = None if null_buf else buf.ptr
        if queued:
            check(ctx.L.bcfgpu_compact_calls_async(ctx.h, n_sites, site0, d_ms, C.byref(co), n_gt_planes, mode, d_buf, cap, cnt.ptr))
            rc = ctx.L.bcfgpu_compact_counts(ctx.h, cnt.ptr, C.byref(nb), C.byref(nr))
            counts = cnt.download(np.zeros(4, np.uint64))
        else:
            rc = ctx.L.bcfgpu_compact_calls(ctx.h, n_sites, site0, d_ms, C.byref(co), n_gt_planes, mode, d_buf, cap, C.byref(nb), C.byref(nr))
        ctx.sync()
        got = buf.download(np.zeros(max(alloc, 16), np.uint8))[:alloc]
    finally:
        ctx.release([buf, cnt])
    return rc, int(nb.value), int(nr.value), got, counts


def assert_matches_packer(ctx, p, mode, with_ms, queued, cap=None):
    want, n_rec = p.want(mode, with_ms)
    alloc = len(want) + SLACK
    rc, nb, nr, got, counts = run_compact(ctx, p.n_sites, p.co, p.d_ms if with_ms else None, p.n_gt_planes, mode,
                                          alloc if cap is None else cap, alloc, queued)
    assert rc == 0 and (nb, nr) == (len(want), n_rec)
    if queued:
        assert [int(x) for x in counts[:3]] == [len(want), n_rec, 0]
    if got[:nb].tobytes() != want:
        bad = np.nonzero(got[:nb] != np.frombuffer(want, np.uint8))[0]
        raise AssertionError("%d bytes differ from the packer's, the first at %d: got 0x%02x, want 0x%02x"
                             % (len(bad), bad[0], got[bad[0]], want[bad[0]]))
    assert (got[nb:] == FILL).all(), "bytes behind the records were written"
    return want, n_rec


@pytest.fixture(scope="module")
def ctx_of(gpu_ctx_factory):
    made = {}

    def get(n_smpl):
        if n_smpl not in made:
            made[n_smpl] = gpu_ctx_factory(abi.default_cfg(n_smpl, max_sites=1024, max_reads=64))
        return made[n_smpl]
    return get


def _pin_one_kept(cs):
    cs["ret"], cs["nals_new"], cs["pl_dropped"] = 2, 2, 0


@pytest.fixture(scope="module")
def planes_of(ctx_of):
    made = {}

    def get(n_sites, n_smpl, n_gt_planes=15):
        key = (n_sites, n_smpl, n_gt_planes)
        if key not in made:
            made[key] = Planes(ctx_of(n_smpl), 31 * n_sites + n_smpl + n_gt_planes, n_sites, n_smpl, n_gt_planes,
                               pin=_pin_one_kept if n_sites == 1 else None)
        return made[key]
    yield get
    for p in made.values():
        p.free()


# ---- A ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n_sites,n_smpl,n_gt_planes", [s + (15,) for s in SHAPES] + [(40, 64, 21)])
def test_compaction_matches_the_packer(ctx_of, planes_of, n_sites, n_smpl, n_gt_planes, mode):
    p = planes_of(n_sites, n_smpl, n_gt_planes)
    if n_sites == 1:
        assert p.want(mode)[1] == 1
    else:
        assert_case_is_telling(p.cs, mode)
    assert (np.array([callrec.n_gt_of(c) for c in p.cs]) <= n_gt_planes).all()
    ctx = ctx_of(n_smpl)
    for with_ms in (True, False):
        a = assert_matches_packer(ctx, p, mode, with_ms, queued=False)
        b = assert_matches_packer(ctx, p, mode, with_ms, queued=True)
        assert a == b
    recs = callrec.walk(a[0], n_smpl)
    assert len(recs) == a[1] and [int(h["site"]) for h, _, _ in recs] == [SITE0 + int(k) for k in np.nonzero(callrec.selected(p.cs, mode))[0]]


@pytest.mark.parametrize("queued", [False, True])
@pytest.mark.parametrize("mode,ret", [(0, -1), (1, 0), (2, 1)])
def test_a_tile_that_compacts_to_nothing(ctx_of, mode, ret, queued):
    def pin(cs):
        cs["ret"], cs["nals_new"], cs["pl_dropped"] = ret, max(ret, 0), 1
    ctx = ctx_of(3)
    p = Planes(ctx, 5, 300, 3, 15, pin=pin)
    try:
        assert p.want(mode) == (b"", 0)
        rc, nb, nr, got, _ = run_compact(ctx, p.n_sites, p.co, p.d_ms, 15, mode, 4096, 4096, queued)
        assert (rc, nb, nr) == (0, 0, 0) and (got == FILL).all()
        # as a size query: nothing to write is no error
        rc, nb, nr, got, _ = run_compact(ctx, p.n_sites, p.co, p.d_ms, 15, mode, 0, 64, queued, null_buf=True)
        assert (rc, nb, nr) == (0, 0, 0) and (got == FILL).all()
    finally:
        p.free()


@pytest.mark.parametrize("queued", [False, True])
def test_no_sites(ctx_of, planes_of, queued):
    p = planes_of(40, 64)
    rc, nb, nr, got, counts = run_compact(ctx_of(64), 0, p.co, p.d_ms, 15, 0, 4096, 4096, queued)
    assert (rc, nb, nr) == (0, 0, 0) and (got == FILL).all()
    if queued:
        assert not counts[:3].any()


# ---- B ---------------------------------------------------------------------------------------------------------------------------
def test_capacity_contract(ctx_of, planes_of):
    ctx, p = ctx_of(64), planes_of(40, 64)
    want, n_rec = p.want(0)
    total = len(want)
    assert n_rec > 1 and total > 16
    for queued in (False, True):
        # sixteen bytes short: refused, the size reported, nothing written
        rc, nb, nr, got, counts = run_compact(ctx, p.n_sites, p.co, p.d_ms, 15, 0, total - 16, total + SLACK, queued)
        assert rc == abi.E_RANGE and (nb, nr) == (total, n_rec)
        assert (got == FILL).all(), "a refused compaction wrote to the buffer"
        if queued:
            assert int(counts[0]) == total and int(counts[1]) == n_rec and int(counts[2]) != 0
        # the size query
        rc, nb, nr, got, _ = run_compact(ctx, p.n_sites, p.co, p.d_ms, 15, 0, 0, 64, queued, null_buf=True)
        assert rc == abi.E_RANGE and (nb, nr) == (total, n_rec) and (got == FILL).all()
        # exactly enough; the context is as usable as before
        assert_matches_packer(ctx, p, 0, True, queued, cap=total)
    assert_matches_packer(ctx, p, 2, True, False)


# ---- C ---------------------------------------------------------------------------------------------------------------------------
def _compact_modes(ctx, n_sites, co, d_ms, n_gt_planes, fill):
    """The records of modes 0 and 2 from planes in HBM, into buffers pre-filled with `fill`."""
    out = {}
    for mode in (0, 2):
        cap = 8 << 20
        buf = ctx.to_device(np.full(cap, fill, np.uint8))
        nb, nr = C.c_uint64(), C.c_uint32()
        try:
            check(ctx.L.bcfgpu_compact_calls(ctx.h, n_sites, SITE0, d_ms, C.byref(co), n_gt_planes, mode, buf.ptr, cap, C.byref(nb), C.byref(nr)))
            ctx.sync()
            out[mode] = (buf.download(np.zeros(cap, np.uint8))[:int(nb.value)].copy(), int(nr.value))
        finally:
            ctx.release([buf])
    return out


def _first_difference(a, b, n_smpl):
    """Where two runs' records differ, in words a reader can follow."""
    if len(a) != len(b):
        return "sizes %d and %d" % (len(a), len(b))
    bad = np.nonzero(a != b)[0]
    o = 0
    for h, _, _ in callrec.walk(a, n_smpl):
        if o + int(h["bytes"]) > bad[0]:
            return "%d bytes differ, the first at offset %d of the record of site %d (ret %d, nals_new %d, n_gt %d, %d bytes)" % (
                len(bad), bad[0] - o, int(h["site"]) - SITE0, int(h["call"]["ret"]), int(h["call"]["nals_new"]), int(h["n_gt"]), int(h["bytes"]))
        o += int(h["bytes"])


MCALL_SEED, MCALL_SITES, MCALL_SMPL = 3, 40, 33


def test_mcall_records_do_not_depend_on_the_buffers(gpu_ctx_factory):
    cin = random_records(MCALL_SEED, MCALL_SITES, MCALL_SMPL, False, 1, False)
    cfg = abi.default_cfg(MCALL_SMPL, max_sites=MCALL_SITES, max_reads=64, call_flag=abi.CALL_VARONLY, output_tags=abi.CALL_FMT_PV4)
    want = orc.mcall(cfg, cin)
    n_skipped, n_live = int((want.site["ret"] == 0).sum()), int((want.site["ret"] > 0).sum())
    assert n_skipped >= 5 and n_live >= 5, (n_skipped, n_live)
    ctx = gpu_ctx_factory(cfg)
    runs = {}
    for fill in (0x00, FILL):
        co, cb, res = ctx.mcall_device(cin, fill=fill)
        try:
            runs[fill] = (res, _compact_modes(ctx, cin.n_sites, co, None, cin.n_gt_max, fill))
        finally:
            ctx.release(list(cb.values()))
    (r0, c0), (r1, c1) = runs[0x00], runs[FILL]
    assert_call_equal(r1, want, MCALL_SMPL)
    assert r0.site.tobytes() == r1.site.tobytes(), "the call records depend on what the buffer held"
    for mode in (0, 2):
        assert c0[mode][1] == c1[mode][1] == int(callrec.selected(want.site, mode).sum())
        assert c0[mode][0].tobytes() == c1[mode][0].tobytes(), "mode %d: %s" % (mode, _first_difference(c0[mode][0], c1[mode][0], MCALL_SMPL))
        # and they are the packer's, from the planes the run left
        assert c1[mode][0].tobytes() == callrec.pack(r1.site, r1.gt, r1.pl, MCALL_SMPL, cin.n_gt_max, SITE0, mode)[0]


def test_pipeline_records_do_not_depend_on_the_buffers(gpu_ctx_factory):
    n_sites, n_smpl = 96, 40
    tile = synth.numpy_tile(4242, n_sites, n_smpl, depth=18.0, var_rate=0.3)
    ctx = gpu_ctx_factory(abi.default_cfg(n_smpl, max_sites=n_sites, max_reads=len(tile.rd) + 64))
    runs = {}
    for fill in (0x00, FILL):
        dt, tb = ctx.upload_tile(tile)
        mo, mb, mres = ctx.alloc_mplp_out(n_sites)
        co, cb, cres = ctx.alloc_call_out(n_sites, abi.MAX_PL)
        try:
            for b in list(mb.values()) + list(cb.values()):
                check(ctx.L.bcfgpu_memset(ctx.h, b.ptr, fill, b.nbytes))
            check(ctx.L.bcfgpu_pipeline(ctx.h, C.byref(dt), None, None, C.byref(mo), C.byref(co)))
            ctx.sync()
            ctx._download(mb, mres)
            ctx._download(cb, cres)
            runs[fill] = (mres, cres, _compact_modes(ctx, n_sites, co, mo.site, abi.MAX_PL, fill))
        finally:
            ctx.release(tb + list(mb.values()) + list(cb.values()))
    (m0, r0, c0), (m1, r1, c1) = runs[0x00], runs[FILL]
    assert m0.site.tobytes() == m1.site.tobytes(), "the site records depend on what the buffer held"
    assert r0.site.tobytes() == r1.site.tobytes(), "the call records depend on what the buffer held"
    for mode in (0, 2):
        assert c0[mode][1] == c1[mode][1] == int(callrec.selected(r1.site, mode).sum()) > 5
        assert c0[mode][0].tobytes() == c1[mode][0].tobytes(), "mode %d: %s" % (mode, _first_difference(c0[mode][0], c1[mode][0], n_smpl))
        assert c1[mode][0].tobytes() == callrec.pack(r1.site, r1.gt, r1.pl, n_smpl, abi.MAX_PL, SITE0, mode, m1.site)[0]


# ---- D ---------------------------------------------------------------------------------------------------------------------------
def test_gather_over_one_rank(ctx_of, gpu_ctx_factory):
    ctx = ctx_of(3)
    L = ctx.L
    comm = C.c_void_p()
    check(L.bcfgpu_comm_init_all((C.c_void_p * 1)(ctx.h.value), 1, C.byref(comm)))
    assert comm.value
    n = 1000
    data = np.random.default_rng(11).integers(0, 256, n, dtype=np.uint8)
    send, recv = ctx.to_device(data), ctx.to_device(np.full(n + SLACK, FILL, np.uint8))
    try:
        check(L.bcfgpu_gather_bytes(comm, 0, send.ptr, (C.c_uint64 * 1)(n), recv.ptr))
        ctx.sync()
        got = recv.download(np.zeros(n + SLACK, np.uint8))
        assert got[:n].tobytes() == data.tobytes() and (got[n:] == FILL).all()
        # in place: nothing to do, nothing changes
        check(L.bcfgpu_gather_bytes(comm, 0, send.ptr, (C.c_uint64 * 1)(n), send.ptr))
        ctx.sync()
        assert send.download(np.zeros(n, np.uint8)).tobytes() == data.tobytes()
        # nothing to gather
        check(L.bcfgpu_gather_bytes(comm, 0, None, (C.c_uint64 * 1)(0), None))
        # a rank the communicator does not have
        assert L.bcfgpu_gather_bytes(comm, 1, send.ptr, (C.c_uint64 * 1)(n), recv.ptr) == abi.E_ARG
    finally:
        L.bcfgpu_comm_destroy(comm)
        ctx.release([send, recv])
    # RCCL wants a device per rank: two contexts on one device are refused before it is loaded
    other = gpu_ctx_factory(abi.default_cfg(3, max_sites=16, max_reads=64))
    comm2 = C.c_void_p(1)
    assert L.bcfgpu_comm_init_all((C.c_void_p * 2)(ctx.h.value, other.h.value), 2, C.byref(comm2)) == abi.E_ARG
    assert not comm2.value
