"""bcfgpu_gap_prep and bcfgpu_pileup + bcfgpu_gap_prep_tile on the designed inputs of tests/helpers/gapgen.py -- general CIGARs,
reads of mixed length shared between columns, repeats, N / lower-case / IUPAC reference letters, contig edges, columns at the
70 % consensus mask, up to 71 indel types, ZQ bytes, insertions past the output capacity -- against the oracle's
bcf_call_gap_prep site by site, every output exact.  tests/test_gap_general_inputs.py shows on the CPU that the inputs are
valid and reach those branches."""
import numpy as np
import pytest

from bcftools_amd import abi
from tests.helpers import gapgen, indeldrv

pytestmark = pytest.mark.gpu

SEEDS = (11, 12)
KEYS = ("ret", "aux", "indel_types", "inscns", "maxins", "indelreg", "max_support", "max_frac")


def batch_against_oracle(ctx, b):
    """bcfgpu_gap_prep for every run of the scenario, checked against the oracle; returns the device results per run."""
    out = []
    for run in b["runs"]:
        got, st = indeldrv.gap_prep_gpu(ctx, b, **run["kw"])
        live = 0
        for k in (range(b["n_sites"]) if run["check"] is None else run["check"]):
            want = indeldrv.gap_prep_oracle_site(b, k, **run["kw"])
            assert (want is None) == (k in run["dead"]), (b["name"], run["kw"], k)
            indeldrv.assert_site_equal(got, k, want)
            live += want is not None
        for k in run["dead"]:
            assert got["ret"][k] < 0
        assert live > 0 and st.n_jobs > 0 and st.dp_cells > 0
        out.append(got)
    return out


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", gapgen.NAMES)
def test_designed_inputs_match_the_oracle_in_both_forms(gpu_ctx_factory, name, seed):
    b = gapgen.scenario(name, seed)
    ctx = gpu_ctx_factory(abi.default_cfg(b["n_smpl"], max_sites=b["n_sites"], max_reads=len(b["p_read"]) + 64))
    got = batch_against_oracle(ctx, b)
    if b["has_unmapped"]:                                  # bcfgpu_pileup takes filtered reads: the same reads, none of them unmapped
        b = gapgen.scenario(name, seed, unmapped=False)
        assert not b["has_unmapped"]
        got = batch_against_oracle(ctx, b)
    # the same reads as a pool: bcfgpu_pileup over the whole contig, then the stage on its columns
    pool = indeldrv.DevicePool(ctx, b, pool=b["pool"])
    col_n, col_indel = gapgen.host_columns(b)
    np.testing.assert_array_equal(pool.col_n, col_n)
    np.testing.assert_array_equal(pool.col_indel, col_indel)
    assert np.array_equal(pool.col_n[pool.cols], np.diff(b["smpl_off"][::b["n_smpl"]])) and pool.col_indel[pool.cols].all()
    for run, g in zip(b["runs"], got):
        got_t, st_t, tile = pool.gap_prep_tile(want_aux=True, **run["kw"])
        indeldrv.assert_tile_matches_host_batch(ctx, b, pool, got_t, tile, g)
        assert tile.n_sites == int((g["ret"] == 0).sum()) > 0


def test_one_context_through_very_different_batches(gpu_ctx_factory):
    """Workspaces sized by a batch of 71-type columns, then reused by batches of other samples, lengths and CIGARs, twice."""
    bs = {n: gapgen.scenario(n, SEEDS[0]) for n in ("manytypes", "repeats", "cigars")}
    cfg = lambda: abi.default_cfg(6, max_sites=16, max_reads=4096)
    fresh = {n: indeldrv.gap_prep_gpu(gpu_ctx_factory(cfg()), bs[n])[0] for n in ("repeats", "cigars")}
    ctx = gpu_ctx_factory(cfg())
    indeldrv.gap_prep_gpu(ctx, bs["manytypes"])
    for rep in range(2):
        for n in ("repeats", "cigars"):
            got, _ = indeldrv.gap_prep_gpu(ctx, bs[n])
            assert (got["ret"] == 0).any()
            for key in KEYS:
                np.testing.assert_array_equal(got[key], fresh[n][key], err_msg="%s %s pass %d" % (n, key, rep))
