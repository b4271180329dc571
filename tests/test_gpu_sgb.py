"""INFO/SGB on the device (combine_kernel's pass over the DP4 planes it has just written) at the edges of its way of summing
calc_SegBias: samples counted by ALT depth 0, 1..511 and from 512 term by term, 256 samples a round, one or four samples
per lane, a cell whose two ALT planes add up past 65 535; and at the regimes of the formula itself (no ALT read, avg_dp = 0,
M clamped either way and on a half, exp(-q) = 0).  Each tile is compared with the oracle and with the math.fsum twin;
tests/test_oracle_sgb.py asserts on the CPU what the tiles reach and which mistakes they could show."""
import numpy as np
import pytest

from tests.helpers import sgbstats as sg
from tests.helpers import sitestats as ss
from tests.test_gpu_parity import assert_mplp_equal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("indel", [False, True])
@pytest.mark.parametrize("n_smpl", sg.SAMPLE_COUNTS)
def test_sgb_at_regime_edges(gpu_ctx_factory, n_smpl, indel):
    """Twice on one context: the second run starts from what the first left in the context's workspace.  The cell of 40 000
    forward and 30 000 reverse ALT reads is within what the library takes (either count fits its 16-bit plane)."""
    tile, cfg, want = sg.sgb_case(n_smpl, indel)
    sg.assert_sgb_coverage(tile)
    tw = ss.twin_seg_bias(tile).astype(np.float64)
    ctx = gpu_ctx_factory(cfg)
    for _ in range(2):
        got = ctx.mpileup(tile)
        assert_mplp_equal(got, want)
        g = got.site["seg_bias"].astype(np.float64)
        assert np.array_equal(np.isposinf(g), np.isposinf(tw)) and not np.isnan(g).any() and not np.isneginf(g).any()
        m = ~np.isinf(tw)
        np.testing.assert_allclose(g[m], tw[m], rtol=ss.RTOL, atol=ss.ATOL, err_msg="twin seg_bias")
