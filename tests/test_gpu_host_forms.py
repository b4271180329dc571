"""The host-pointer forms of the read stages (bcfgpu_baq, bcfgpu_cap_mapq, bcfgpu_overlap_tweak) as fronts of the pool forms'
cores: they upload the caller's reads as a view and run the same code the context's pool goes through.  What that must not
change: a host-form call leaves the pool and its BAQ results alone, the arrays a stage does not read stay optional, and the
fronts' edge cases (no reads; reads BAQ leaves alone, so that there is no reference slice to upload) behave as before."""
import ctypes as C

import numpy as np
import pytest

from bcftools_amd import abi, engine, synth
from bcftools_amd.lib import check
from tests.helpers import mplpdrv as M
from tests.test_gpu_baq import _random_reads
from tests.test_gpu_pileup import assert_tiles_equal
from tests.test_gpu_pool import _tile_of

pytestmark = pytest.mark.gpu

READ_KEYS = ("r_pos", "r_lq", "r_flag", "r_ncig", "r_cig_off", "r_seq_off", "cig", "seq16", "qual", "zq", "r_has_zq")
S = 20


def _struct(reads):
    rd = abi.Reads()
    rd.n_reads = reads["n_reads"]
    for k in READ_KEYS:
        setattr(rd, k, reads[k].ctypes.data)
    return rd


def _pool_baq(ctx, b):
    """bcfgpu_pool_upload -> bcfgpu_pool_baq; returns the pool's reads and r_smpl."""
    reads, mapq, smpl, _ = synth.indel_pool(b)
    check(ctx.L.bcfgpu_pool_upload(ctx.h, C.byref(_struct(reads)), None, mapq.ctypes.data))
    check(ctx.L.bcfgpu_pool_baq(ctx.h, b["ref"], len(b["ref"]), 3, None))
    return reads, smpl


def _download(ctx, reads):
    nb, n = len(reads["qual"]), int(reads["n_reads"])
    q, z, m = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8), np.zeros(n, np.uint8)
    check(ctx.L.bcfgpu_pool_download(ctx.h, q.ctypes.data, z.ctypes.data, m.ctypes.data))
    return q, z, m


def _pileup(ctx, b, smpl):
    t = abi.Tile()
    L = len(b["ref"])
    check(ctx.L.bcfgpu_pool_pileup(ctx.h, smpl.ctypes.data, None, 0, L, b["ref"], L, C.byref(t), None, None))
    return _tile_of(ctx, t, L, S)


def _host_forms(ctx, b):
    """The three host-pointer calls on the reads of `b`; returns their outputs."""
    reads, _, _, _ = synth.indel_pool(b)
    rd = _struct(reads)
    n, nb = int(reads["n_reads"]), len(reads["qual"])
    q, z, ret = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8), np.zeros(n, np.int32)
    check(ctx.L.bcfgpu_baq(ctx.h, C.byref(rd), b["ref"], len(b["ref"]), 3, q.ctypes.data, z.ctypes.data, ret.ctypes.data))
    cap = np.zeros(n, np.int32)
    check(ctx.L.bcfgpu_cap_mapq(ctx.h, C.byref(rd), b["ref"], len(b["ref"]), 50, cap.ctypes.data))
    pa, pb = np.arange(0, n - 1, 2, dtype=np.int32), np.arange(1, n, 2, dtype=np.int32)
    q2 = np.zeros(nb, np.uint8)
    check(ctx.L.bcfgpu_overlap_tweak(ctx.h, C.byref(rd), len(pa), pa.ctypes.data, pb.ctypes.data, q2.ctypes.data))
    return q, z, ret, cap, q2


def test_host_form_calls_leave_the_pools_baq_results_alone():
    """Both fronts of a stage run one core: the host form's outputs and scratch must be none of the slots the context's pool keeps
    its qualities, ZQ bytes and flags in.  A pool with reads of all four band classes through bcfgpu_pool_baq; then the three
    host forms on another batch (more reads: the buffers they share with the cores regrow); the pool reads back, and piles up,
    as it does on a context that never saw those calls.  And the other way round: the host forms first."""
    a = synth.indel_batch(77, 6, S, depth=12.0, lens=(-40, -25, -12, -8, 8, 12, 25, 40), lens2=(-3, 2, 60, -90))
    other = synth.indel_batch(78, 9, S, depth=16.0, lens=(-30, -9, 3, 10), lens2=(-2, 1, 45))
    assert other["reads"]["n_reads"] > a["reads"]["n_reads"] > 1000
    cfg = abi.default_cfg(S, max_sites=1, max_reads=64)
    with engine.Context(cfg) as ctx:
        reads, smpl = _pool_baq(ctx, a)
        want = _download(ctx, reads)
        want_tile = _pileup(ctx, a, smpl)
        want_host = _host_forms(ctx, other)
    assert (want[0] != reads["qual"]).any() and want[1].any()
    with engine.Context(cfg) as ctx:
        reads, smpl = _pool_baq(ctx, a)
        first = _download(ctx, reads)
        got_host = _host_forms(ctx, other)
        again = _download(ctx, reads)
        tile = _pileup(ctx, a, smpl)
    for x, y, w in zip(first, again, want):
        assert x.tobytes() == w.tobytes() and y.tobytes() == w.tobytes()
    assert_tiles_equal(tile, want_tile)
    for x, w in zip(got_host, want_host):
        assert x.tobytes() == w.tobytes()
    with engine.Context(cfg) as ctx:
        got_host = _host_forms(ctx, other)
        reads, smpl = _pool_baq(ctx, a)
        got = _download(ctx, reads)
        tile = _pileup(ctx, a, smpl)
    for x, w in zip(got, want):
        assert x.tobytes() == w.tobytes()
    assert_tiles_equal(tile, want_tile)
    for x, w in zip(got_host, want_host):
        assert x.tobytes() == w.tobytes()


def test_arrays_a_stage_does_not_read_stay_optional(gpu_ctx_factory):
    """bcfgpu_cap_mapq and bcfgpu_overlap_tweak read neither r_flag nor zq / r_has_zq: with those NULL they give what they give
    with every member set."""
    refseq, reads = _random_reads(105, 64)
    ctx = gpu_ctx_factory(abi.default_cfg(1, max_sites=1, max_reads=64))
    n = len(reads)
    pa, pb = np.arange(0, n, 2, dtype=np.int32), np.arange(1, n, 2, dtype=np.int32)

    def run(strip):
        rd, d = M.pack_reads(reads)
        if strip:
            rd.r_flag = rd.zq = rd.r_has_zq = None
        cap, q = np.full(n, -7, np.int32), np.full(len(d["qual"]), 0xAA, np.uint8)
        check(ctx.L.bcfgpu_cap_mapq(ctx.h, C.byref(rd), refseq.encode(), len(refseq), 50, cap.ctypes.data))
        check(ctx.L.bcfgpu_overlap_tweak(ctx.h, C.byref(rd), len(pa), pa.ctypes.data, pb.ctypes.data, q.ctypes.data))
        return cap, q, d["qual"]
    cap, q, q_in = run(False)
    cap_s, q_s, _ = run(True)
    np.testing.assert_array_equal(cap_s, cap)
    np.testing.assert_array_equal(q_s, q)
    assert (cap != -7).all() and (q != q_in).any() and (q != 0xAA).any()


def test_host_forms_without_reads_write_nothing(gpu_ctx_factory):
    ctx = gpu_ctx_factory(abi.default_cfg(1, max_sites=1, max_reads=64))
    rd = abi.Reads()
    q, z = np.full(8, 0xAA, np.uint8), np.full(8, 0xAA, np.uint8)
    ret, cap = np.full(8, -7, np.int32), np.full(8, -7, np.int32)
    check(ctx.L.bcfgpu_baq(ctx.h, C.byref(rd), b"ACGTACGT", 8, 3, q.ctypes.data, z.ctypes.data, ret.ctypes.data))
    check(ctx.L.bcfgpu_cap_mapq(ctx.h, C.byref(rd), b"ACGTACGT", 8, 50, cap.ctypes.data))
    check(ctx.L.bcfgpu_overlap_tweak(ctx.h, C.byref(rd), 0, None, None, q.ctypes.data))
    assert (q == 0xAA).all() and (z == 0xAA).all() and (ret == -7).all() and (cap == -7).all()


def _left_alone(cause, reads):
    for r in reads:
        if cause == "no qualities":
            r.qual[0] = 0xff
        elif cause == "unmapped":
            r.flag = 4
        elif cause == "N in CIGAR":
            a = r.l_qseq // 2
            r.bamcigar = np.array([a << 4 | 0, 5 << 4 | 3, (r.l_qseq - a) << 4 | 0], dtype=np.uint32)
        else:
            r.bamcigar = np.array([10 << 4 | 4, (r.l_qseq - 10) << 4 | 1], dtype=np.uint32)      # soft clip and insertion: no aligned base


@pytest.mark.parametrize("cause", ["no qualities", "unmapped", "N in CIGAR", "no aligned base"])
def test_baq_on_reads_it_leaves_alone(gpu_ctx_factory, cause):
    """Every read with sam_prob_realn's ret = -1, for one of its causes: the qualities come back as they went in, no ZQ byte, and
    no window asks for a reference slice (the lowest window start stays at its initial value)."""
    refseq, reads = _random_reads(106, 48)
    _left_alone(cause, reads)
    ctx = gpu_ctx_factory(abi.default_cfg(1, max_sites=1, max_reads=64))
    rd, d = M.pack_reads(reads)
    nb, n = len(d["qual"]), len(reads)
    q, z, ret = np.full(nb, 0xAA, np.uint8), np.full(nb, 0xAA, np.uint8), np.full(n, 7, np.int32)
    check(ctx.L.bcfgpu_baq(ctx.h, C.byref(rd), refseq.encode(), len(refseq), 3, q.ctypes.data, z.ctypes.data, ret.ctypes.data))
    np.testing.assert_array_equal(q, d["qual"])
    assert not z.any() and (ret == -1).all()
