"""The stand-alone caller (bcfgpu_mcall: int32 PLs as parsed from a VCF/BCF) against the oracle at cohort scale with PLs
over their whole range, and both caller paths on data with exact ties.

PLs past 255 leave set_pdg's table for pow(10, -PL/10) (mcall.c:472, 491), subnormal from PL 3077 and 0 from 3237: the
records of tests/helpers/mcallgen.cohort_records() hold such entries in both places, from a per-read error model at depth
120 and as explicit edge values.  The tie records and tiles are symmetric under swapping two ALT alleles, so a tie between a
subset and its mirror, or between two genotypes, is exact under any arithmetic; the reference keeps the first maximum in its
visiting order (mcall.c:583, strict `best_lk < lk` for genotypes) and orders equal-QS ALTs by a stable ascending sort walked
from the top (bam2bcf.c:578-598).  Those rules are asserted here directly as well as through the oracle."""
import numpy as np
import pytest

from bcftools_amd import abi, host
from tests.helpers import orc
from tests.helpers import mcallgen as mg
from tests.test_gpu_parity import assert_call_equal, assert_mplp_equal

pytestmark = pytest.mark.gpu

ALL_TAGS = abi.CALL_FMT_GQ | abi.CALL_FMT_GP | abi.CALL_FMT_PV4


def assert_gq_gp_equal(got, want, tags):
    """GQ exact, GP to 1e-5 relative (as tests/test_gpu_mcall_random.py), at the called variant records."""
    live = (want.site["ret"] > 0) & (want.site["als_new"] != 1)
    if tags & abi.CALL_FMT_GQ:
        np.testing.assert_array_equal(got.gq[live], want.gq[live])
    if tags & abi.CALL_FMT_GP:
        for i in np.nonzero(live)[0]:
            nn = int(want.site["nals_new"][i])
            ng = nn * (nn + 1) // 2
            g, w = got.gp[i, :ng], want.gp[i, :ng]
            assert np.array_equal(np.isnan(g), np.isnan(w))
            np.testing.assert_allclose(g[~np.isnan(w)], w[~np.isnan(w)], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("seed,n_sites,n_smpl,use_ploidy,n_grp,shuffled,use_prior,flags", [
    (101, 24, 64, False, 1, False, False, 0),
    (102, 24, 65, True, 1, False, True, 0),
    (103, 15, 255, False, 3, False, False, abi.CALL_VARONLY),
    (104, 15, 256, True, 3, True, True, 0),
    (105, 15, 257, False, 13, True, False, abi.CALL_KEEPALT),
    (106, 12, 1000, True, 13, False, True, 0),
    (107, 12, 1001, False, 1, False, False, 0),
    (108, 9, 4100, True, 3, True, False, 0),
])
def test_cohort_records_match_oracle(gpu_ctx_factory, seed, n_sites, n_smpl, use_ploidy, n_grp, shuffled, use_prior, flags):
    cin = mg.cohort_records(seed, n_sites, n_smpl, use_ploidy, n_grp, shuffled, use_prior)
    assert cin.n_gt_max == 15 or n_sites < 5
    pl = cin.pl[(cin.pl != abi.INT32_MISSING) & (cin.pl != abi.INT32_VECTOR_END)]
    assert (pl >= 256).sum() > 50 and ((pl >= mg.PL_SUBNORMAL) & (pl < mg.PL_ZERO)).any() and (pl >= mg.PL_ZERO).any()
    cfg = abi.default_cfg(n_smpl, max_sites=n_sites, call_flag=flags, output_tags=ALL_TAGS, n_grp=n_grp)
    want = orc.mcall(cfg, cin)
    got = gpu_ctx_factory(cfg).mcall(cin)
    assert_call_equal(got, want, n_smpl)
    assert_gq_gp_equal(got, want, ALL_TAGS)
    kept = want.site["nals_new"][want.site["ret"] > 0]
    assert (kept >= 2).sum() >= 3 and (kept >= 3).any()


@pytest.mark.parametrize("n_smpl,use_ploidy,n_grp,shuffled", [
    (40, False, 1, False), (64, True, 1, False), (257, False, 1, False), (1001, True, 1, False),
    (100, False, 3, False), (130, True, 3, True), (300, False, 13, True), (301, True, 13, False),
])
def test_tie_records_match_oracle(gpu_ctx_factory, n_smpl, use_ploidy, n_grp, shuffled):
    """Every tie kind of mcallgen.TIE_KINDS (the 3-, 15- and 25-subset instantiations, an allele of frequency 0 before the
    tied pair, the unseen allele), with sample groups on AD that are equal for the tied alleles."""
    cin, kinds = mg.tie_records(7 + n_smpl, n_smpl, use_ploidy=use_ploidy, n_grp=n_grp, shuffled=shuffled)
    cfg = abi.default_cfg(n_smpl, max_sites=cin.n_sites, output_tags=ALL_TAGS, n_grp=n_grp)
    want = orc.mcall(cfg, cin)
    got = gpu_ctx_factory(cfg).mcall(cin)
    assert_call_equal(got, want, n_smpl)
    assert_gq_gp_equal(got, want, ALL_TAGS)
    for k, kind in enumerate(kinds):
        lo, hi = mg.TIE_KINDS[kind][3]
        als = int(got.site["als_new"][k])
        if kind == "gt":
            assert als & (1 << lo) and als & (1 << hi)
        else:
            assert als & (1 << lo) and not als & (1 << hi), (kind, bin(als))
        # a sample whose likelihoods are symmetric never gets the later allele of the pair (genotypes: strict best_lk < lk)
        sym = mg.symmetric_samples(cin, k, lo, hi)
        assert not mg.later_without_earlier(got.gt[k][:, sym], got.site["als_map"][k], lo, hi).any()
        if kind == "gt":
            lm = int(got.site["als_map"][k][lo])
            assert (got.gt[k][:, sym] == lm).sum() > n_smpl // 8


@pytest.mark.parametrize("n_sites,n_smpl,use_ploidy,n_grp,runs,ref_n", [
    (24, 100, False, 1, False, False),        # one sample a lane
    (16, 200, False, 1, False, False),        # four samples a lane
    (16, 300, False, 1, False, False),        # with many samples the three-allele sites run in the 15-subset instantiation
    (16, 100, True, 1, False, False),         # HAP
    (16, 200, True, 1, False, False),
    (12, 120, False, 1, False, True),         # an N reference: five alleles
    (12, 260, True, 1, False, True),
    (16, 120, False, 12, True, False),        # GRP: up to 12 groups batched on the 64 lanes
    (16, 150, True, 12, False, False),
    (16, 130, False, 13, True, False),        # 13 groups: the general group path
    (12, 260, True, 13, False, True),
])
def test_pipeline_ties_match_oracle(gpu_ctx_factory, n_sites, n_smpl, use_ploidy, n_grp, runs, ref_n):
    """The fused pipeline on mcallgen.tie_tile(): two non-reference bases with equal QS at every site.  The higher base is
    the first ALT (bam2bcf.c:578-598), its PL planes mirror the lower one's, and the caller keeps the first ALT of a tied
    subset pair and the first of two tied genotypes.  (Two ALTs of a known reference base always bring <*>, so such a site has
    at least four alleles: the 3-allele instantiation sees no ALT tie here; test_tie_records_match_oracle covers it.)"""
    tile, lo, hi = mg.tie_tile(n_sites * 1000 + n_smpl + n_grp, n_sites, n_smpl, ref_n=ref_n)
    fmt = abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD
    cfg = abi.default_cfg(n_smpl, max_sites=n_sites, max_reads=len(tile.rd), fmt_flag=fmt, n_grp=n_grp,
                          output_tags=abi.CALL_FMT_GQ)
    rng = np.random.default_rng(n_smpl)
    ploidy = rng.choice([1, 2, 2], size=n_smpl).astype(np.uint8) if use_ploidy else None
    grp = None
    if n_grp > 1:
        grp = (np.arange(n_smpl) * n_grp // n_smpl).astype(np.int32)
        if not runs:
            rng.shuffle(grp)
    mwant = orc.mpileup(cfg, tile)
    na = mwant.site["n_alleles"]
    ad = None
    if n_grp > 1:
        src = mwant.adf.astype(np.int32) + mwant.adr.astype(np.int32)
        ad = np.where(np.arange(5)[None, :, None] < na[:, None, None], src, abi.INT32_VECTOR_END).astype(np.int32)
    cin = host.CallInput(n_smpl, na, np.maximum(mwant.site["unseen"], 0), mwant.pl.astype(np.int32), mwant.site["qsum"],
                         ad=ad, ploidy=ploidy, grp=grp, i16=mwant.site["anno"].astype(np.float32))
    cwant = orc.mcall(cfg, cin)
    mgot, cgot = gpu_ctx_factory(cfg).pipeline(tile, ploidy=ploidy, grp=grp)
    assert_mplp_equal(mgot, mwant)
    assert_call_equal(cgot, cwant, n_smpl)
    assert_gq_gp_equal(cgot, cwant, abi.CALL_FMT_GQ)
    # the reference's rules themselves, on the device's output
    called = 0
    for k in range(n_sites):
        order = list(mgot.site["a"][k])
        j = order.index(hi[k])
        assert order[j + 1] == lo[k]                  # equal QS: the higher base first
        als = int(cgot.site["als_new"][k])
        assert (als >> j) & 1 or not (als >> (j + 1)) & 1
        # every cell holds as many reads of one tied base as of the other
        assert not mg.later_without_earlier(cgot.gt[k], cgot.site["als_map"][k], j, j + 1).any()
        called += (als >> j) & 1
    assert called >= n_sites // 2
