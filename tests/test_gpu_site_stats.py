"""The bias-test histograms and the site statistics at depth: tiles that put more than 65 535 accepted reads of one
workgroup into one bin of one histogram (base quality 40, mapQ 60, one epos value), in every form the kernel keeps the
counts in -- the packed 16-bit halves of the LDS form (one slot, a site over two workgroups, eight slots, the workgroup of
a listed deep cell, the indel instantiation) and, as a control, the 32-bit global form.  Each tile is compared with the
oracle and with the numpy twin of tests/helpers/sitestats.py; tests/test_oracle_site_stats.py asserts, on the CPU, that
each tile's statistics would change if a counter wrapped."""
import numpy as np
import pytest

from tests.helpers import sitestats as ss
from tests.test_gpu_parity import assert_mplp_equal

pytestmark = pytest.mark.gpu


def _assert_twin(got, tile):
    tw = ss.twin_stats(tile)
    for k in ss.STATS + ("seg_bias",):
        g, w = got.site[k].astype(np.float64), tw[k].astype(np.float64)
        assert np.array_equal(np.isinf(g), np.isinf(w)), k
        m = ~np.isinf(w)
        np.testing.assert_allclose(g[m], w[m], rtol=ss.RTOL, atol=ss.ATOL, err_msg="twin " + k)
    np.testing.assert_array_equal(got.sp, ss.twin_sp(tile), err_msg="twin sp")


@pytest.mark.parametrize("name", list(ss.DEEP_CASES))
def test_histograms_at_depth(gpu_ctx_factory, name):
    """Twice on one context: the second run starts from what the first left in the context's workspace."""
    tile, cfg, want = ss.deep_case(name)
    ctx = gpu_ctx_factory(cfg)
    for _ in range(2):
        got = ctx.mpileup(tile)
        assert_mplp_equal(got, want)
        _assert_twin(got, tile)


@pytest.mark.parametrize("n_smpl", [3, 48, 0])
def test_regimes_of_the_statistics(gpu_ctx_factory, n_smpl):
    """Part B: sites that walk every branch of calc_mwu_bias (0, 1, 2, the exact table for 3..7 with whole and half-integer
    U and complete separation either way, the normal approximation from 8), of calc_vdb (fewer than 2 reads, 2, depths on,
    between and past the table's rows) and of FMT/SP (each margin at 0 and 1, walks over n11 = 11, 22, 33, cells past 255
    reads, the cap at 255), in the global form (3 samples) and in the LDS form (48).  n_smpl 0: the tile of 64 samples whose
    sum of pos * i passes 2^24, where calc_vdb's float sum has to be replayed in order.  The coverage is asserted, so a
    change to the generator cannot quietly lose a regime."""
    tile, cfg, want = ss.regime_case(n_smpl)
    if n_smpl:
        ss.assert_regime_coverage(tile)
    else:
        assert "replay" in ss.vdb_regimes(ss.site_hists(tile, 0)["alt_pos"])
    got = gpu_ctx_factory(cfg).mpileup(tile)
    assert_mplp_equal(got, want)
    _assert_twin(got, tile)
