"""The caller's prior under cfg.ploidy_max on the device (csrc/api.hip: n = ploidy_max * n_smpl, mcall.c:396-416 with
vcfcall.c:652-656) against the oracle and against the closed form of tests/helpers/priorrecs.py: ploidy_max 0 (= 2), 1 and 2; 1, 2,
3 and 65 samples; the default prior, none, and 0.2, which at 65 samples stays under the 0.99 cap for ploidy_max 1 and reaches it
for 2; with and without a ploidy array.  bcfgpu_mcall runs on random records with prior-only records among them, bcfgpu_pipeline
on a synthetic tile of 24 sites.  tests/test_oracle_prior_ploidy.py is the half that needs no GPU."""
import numpy as np
import pytest

from bcftools_amd import abi, synth, host
from tests.helpers import orc, priorrecs as PR
from tests.test_gpu_parity import assert_call_equal, assert_mplp_equal
from tests.test_oracle_prior_ploidy import QUAL_TOL, THETAS, SAMPLES, cfg_for, oracle_calls, check_closed_form

pytestmark = pytest.mark.gpu

TILE_SITES = 24
_tiles = {}


def tile_and_planes(n_smpl):
    """The pipeline's tile and the oracle's mpileup planes of it, once per sample count (the mpileup stage does not read the prior)."""
    if n_smpl not in _tiles:
        tile = synth.numpy_tile(500 + n_smpl, TILE_SITES, n_smpl, depth=12.0, var_rate=0.3)
        _tiles[n_smpl] = tile, orc.mpileup(cfg_for(n_smpl, 1.1e-3, 2, TILE_SITES, len(tile.rd)), tile)
    return _tiles[n_smpl]


@pytest.mark.parametrize("use_ploidy", [False, True])
@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_prior_allele_count_on_the_device(gpu_ctx_factory, n_smpl, theta, use_ploidy):
    cin, where, want = oracle_calls(n_smpl, theta, use_ploidy)
    for r in want.values():
        PR.assert_prior_only(r, where)
    if theta == 0.2 and n_smpl == 65:                            # the cap case, from the formula
        assert not PR.scaled_theta(theta, PR.prior_alleles(1, n_smpl))[1] and PR.scaled_theta(theta, PR.prior_alleles(2, n_smpl))[1]
    tile, mwant = tile_and_planes(n_smpl)
    pin = host.CallInput(n_smpl, mwant.site["n_alleles"], np.maximum(mwant.site["unseen"], 0), mwant.pl.astype(np.int32),
                         mwant.site["qsum"], ploidy=cin.ploidy, i16=mwant.site["anno"].astype(np.float32))
    got, pgot = {}, {}
    for pm in (0, 1, 2):
        cfg = cfg_for(n_smpl, theta, pm, max(TILE_SITES, cin.n_sites), len(tile.rd))
        ctx = gpu_ctx_factory(cfg)
        got[pm] = ctx.mcall(cin)
        assert_call_equal(got[pm], want[pm], n_smpl)
        mgot, pgot[pm] = ctx.pipeline(tile, ploidy=cin.ploidy)
        assert_mplp_equal(mgot, mwant)
        assert_call_equal(pgot[pm], orc.mcall(cfg, pin), n_smpl)
    check_closed_form(got, where, theta, n_smpl)
    np.testing.assert_array_equal(pgot[0].site["qual"], pgot[2].site["qual"])
    # the pipeline's records feel the allele count as well: every QUAL that is not 0 or missing moves with it
    if theta > 0 and n_smpl >= 2:
        live = (pgot[2].site["ret"] > 0) & (pgot[2].site["qual_missing"] == 0) & (pgot[2].site["qual"] > 10 * QUAL_TOL)
        assert live.any() and not np.allclose(pgot[1].site["qual"][live], pgot[2].site["qual"][live], rtol=QUAL_TOL, atol=QUAL_TOL)
