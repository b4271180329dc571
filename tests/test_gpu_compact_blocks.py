"""bcfgpu_compact_calls (bcftools_amd/csrc/gather.hip) where its kernels' grids have their edges: the size pass works in blocks of
256 sites, the scan hands every site its offset, the copy pass writes each record where the offsets say.  Against the plain packer
of tests/helpers/callrec.py, byte for byte, into buffers pre-filled with 0xA5 (every byte of every record is shown to be
written, and none behind them):

  - tiles of 1, 255, 256, 257 and 600 sites with 1, 3 and 65 samples, every variants_only mode;
  - the only record of a tile at the first or the last site of a block, every site a record, and none;
  - a skipped site (nals_new == 0: GT is BCFGPU_GT_MISSING) and one with pl_dropped as the only records of their blocks;
  - a capacity one byte short: counts[2] == 1, the size reported, the buffer untouched.
"""
import numpy as np
import pytest

from bcftools_amd import abi
from tests.helpers import callrec
from tests.test_gpu_compact import FILL, SITE0, SLACK, Planes, assert_matches_packer, run_compact

pytestmark = pytest.mark.gpu

SITES, SMPLS = [1, 255, 256, 257, 600], [1, 3, 65]


@pytest.fixture(scope="module")
def ctx_of(gpu_ctx_factory):
    made = {}

    def get(n_smpl):
        if n_smpl not in made:
            made[n_smpl] = gpu_ctx_factory(abi.default_cfg(n_smpl, max_sites=1024, max_reads=64))
        return made[n_smpl]
    return get


def _with_planes(ctx, seed, n_sites, n_smpl, pin, body):
    p = Planes(ctx, seed, n_sites, n_smpl, 15, pin=pin)
    try:
        return body(p)
    finally:
        p.free()


def _pin_one_kept(cs):
    cs["ret"], cs["nals_new"], cs["pl_dropped"] = 2, 2, 0


@pytest.mark.parametrize("n_smpl", SMPLS)
@pytest.mark.parametrize("n_sites", SITES)
def test_random_tiles_in_every_mode(ctx_of, n_sites, n_smpl):
    ctx = ctx_of(n_smpl)

    def body(p):
        for mode in (0, 1, 2):
            keep = callrec.selected(p.cs, mode)
            if n_sites > 1:
                assert keep.any() and (~keep).any()
            for queued in (False, True):
                _, n_rec = assert_matches_packer(ctx, p, mode, True, queued)
                assert n_rec == int(keep.sum())
    _with_planes(ctx, 977 * n_sites + n_smpl, n_sites, n_smpl, _pin_one_kept if n_sites == 1 else None, body)


def _only(sites, ret=2, nals_new=2, pl_dropped=0):
    """Every site REF-only (kept by mode 0 alone) but `sites`, which get the given record."""
    def pin(cs):
        cs["ret"], cs["nals_new"], cs["pl_dropped"] = 0, 0, 1
        for k in sites:
            cs["ret"][k], cs["nals_new"][k], cs["pl_dropped"][k] = ret, nals_new, pl_dropped
    return pin


@pytest.mark.parametrize("n_smpl", SMPLS)
@pytest.mark.parametrize("k", [0, 255, 256, 511, 512, 599])
def test_the_only_variant_at_the_edge_of_a_block(ctx_of, n_smpl, k):
    ctx = ctx_of(n_smpl)

    def body(p):
        for mode in (1, 2):
            want, n_rec = assert_matches_packer(ctx, p, mode, True, True)
            assert n_rec == 1 and int(callrec.walk(want, n_smpl)[0][0]["site"]) - SITE0 == k
        # mode 0: every site has a record, the skipped ones among them
        assert assert_matches_packer(ctx, p, 0, True, False)[1] == 600
    _with_planes(ctx, 40 + k, 600, n_smpl, _only([k]), body)


@pytest.mark.parametrize("n_smpl", SMPLS)
@pytest.mark.parametrize("n_sites", [256, 257, 600])
def test_every_site_a_variant_and_none(ctx_of, n_sites, n_smpl):
    ctx = ctx_of(n_smpl)

    def every(cs):
        cs["ret"] = cs["nals_new"] = 2 + np.arange(n_sites) % 4           # record sizes differ from site to site
        cs["pl_dropped"] = 0

    def body_every(p):
        for mode in (0, 1, 2):
            assert assert_matches_packer(ctx, p, mode, True, True)[1] == n_sites
    _with_planes(ctx, 7, n_sites, n_smpl, every, body_every)

    def body_none(p):
        for mode in (1, 2):
            assert p.want(mode) == (b"", 0)
            rc, nb, nr, got, counts = run_compact(ctx, n_sites, p.co, p.d_ms, 15, mode, 4096, 4096, True)
            assert (rc, nb, nr) == (0, 0, 0) and (got == FILL).all() and not counts[:3].any()
    _with_planes(ctx, 8, n_sites, n_smpl, _only([]), body_none)


@pytest.mark.parametrize("n_smpl", SMPLS)
def test_skipped_and_dropped_pl_records(ctx_of, n_smpl):
    """Blocks 0 and 2 hold one record each: a skipped site whose ret still selects it (no genotype was written: GT missing, no PL),
    and a called site whose PL planes were dropped.  Block 1 holds none."""
    ctx = ctx_of(n_smpl)

    def pin(cs):
        cs["ret"], cs["nals_new"], cs["pl_dropped"] = -1, 0, 0
        cs["ret"][100], cs["nals_new"][100], cs["pl_dropped"][100] = 3, 0, 0
        cs["ret"][530], cs["nals_new"][530], cs["pl_dropped"][530] = 3, 3, 1

    def body(p):
        for mode in (0, 1):
            want, n_rec = assert_matches_packer(ctx, p, mode, True, True)
            (h0, g0, p0), (h1, g1, p1) = callrec.walk(want, n_smpl)
            assert n_rec == 2 and (g0 == abi.GT_MISSING).all() and p0.size == 0 and p1.size == 0
            assert int(h1["call"]["pl_dropped"]) == 1 and (g1 == p.gt[530]).all()
        assert assert_matches_packer(ctx, p, 2, True, True)[1] == 1
    _with_planes(ctx, 9, 600, n_smpl, pin, body)


@pytest.mark.parametrize("n_smpl", SMPLS)
@pytest.mark.parametrize("n_sites", [1, 257, 600])
def test_one_byte_short(ctx_of, n_sites, n_smpl):
    ctx = ctx_of(n_smpl)

    def body(p):
        want, n_rec = p.want(0)
        total = len(want)
        assert n_rec >= 1
        for queued in (False, True):
            rc, nb, nr, got, counts = run_compact(ctx, n_sites, p.co, p.d_ms, 15, 0, total - 1, total + SLACK, queued)
            assert rc == abi.E_RANGE and (nb, nr) == (total, n_rec)
            assert (got == FILL).all(), "a refused compaction wrote to the buffer"
            if queued:
                assert [int(x) for x in counts[:3]] == [total, n_rec, 1]
        # exactly enough
        assert_matches_packer(ctx, p, 0, True, True, cap=total)
    _with_planes(ctx, 11 * n_sites + n_smpl, n_sites, n_smpl, _pin_one_kept if n_sites == 1 else None, body)
