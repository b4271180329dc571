"""DP4, MQ and PV4 from I16 on the device (i16_kernel: four lanes a site, Fisher's walk in one and kf_betai's continued fraction
in the other three) at the regimes of tests/helpers/i16stats.py, on both routes: bcfgpu_mcall with the I16 vectors given, and
bcfgpu_pipeline, where the caller casts the mpileup stage's site sums to float.  Compared with the oracle: the integer
fields, the NaN pattern and the zeros exactly; 2e-6 relative where the value is a normal float; one subnormal step below
that.  tests/test_oracle_i16.py asserts on the CPU what the vectors reach and checks the oracle's test16 itself."""
import numpy as np
import pytest

from tests.helpers import i16stats as i16
from tests.test_gpu_parity import assert_mplp_equal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_sites", [0, 1, 15, 16, 17, 33])
def test_i16_given_to_the_caller(gpu_ctx_factory, n_sites):
    """Records of 1, 15, 16, 17 and 33 sites (a workgroup holds sixteen) and the whole catalog (0), special vectors on either
    side of the workgroup boundaries, skipped records between the called ones.  Twice on one context."""
    names, cin, skipped, cfg, want = i16.mcall_case(n_sites)
    if not n_sites:
        i16.assert_coverage(cin.i16[~skipped])
    ctx = gpu_ctx_factory(cfg)
    for _ in range(2):
        got = ctx.mcall(cin)
        i16.assert_i16_equal(got, want)
        np.testing.assert_array_equal(got.gt[~skipped], want.gt[~skipped])
    st = got.site
    # what the comparison above implies, said once more on the device's own result
    assert np.isnan(st["pv4"]).sum() == sum(k.startswith("neg_var") for k in names)
    assert (st["has_i16"][skipped] == 0).all() and (st["pv4"][skipped] == 0).all() and (st["dp4"][skipped] == 0).all()


def test_pv4_tag_off(gpu_ctx_factory):
    """Without the PV4 tag no site is tested and pv4 stays 0; DP4 and MQ are set all the same."""
    names, cin, skipped, cfg, want = i16.mcall_case(0, 0)
    got = gpu_ctx_factory(cfg).mcall(cin)
    i16.assert_i16_equal(got, want)
    assert (got.site["pv4_tested"] == 0).all() and (got.site["pv4"] == 0).all() and (got.site["has_i16"][~skipped] == 1).all()
    assert (got.site["dp4"].sum(axis=1) > 0).sum() > 40


def test_i16_from_the_mpileup_stage(gpu_ctx_factory):
    """Seventeen sites built from reads, the deep constant-quality site (NaN) and the zero-variance site (exact zeros) at sites
    15 and 16; sites without an ALT read are skipped under CALL_VARONLY.  The stage's I16 are first the intended vectors
    exactly."""
    names, tile, vecs, cfg, mwant, cwant = i16.fused_case()
    i16.assert_coverage(vecs, i16.FUSED_NEED)
    ctx = gpu_ctx_factory(cfg)
    for _ in range(2):
        mgot, cgot = ctx.pipeline(tile)
        np.testing.assert_array_equal(mgot.site["anno"].astype(np.float32), vecs)
        assert_mplp_equal(mgot, mwant)
        i16.assert_i16_equal(cgot, cwant)
    assert np.isnan(cgot.site["pv4"][15, 1]) and cgot.site["pv4"][16].tolist() == [1, 0, 0, 0]
