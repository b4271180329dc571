"""CPU checks behind tests/test_gpu_mcall_cohort.py: its generators reach what they are for, and the oracle follows the
reference's rules on exact ties -- the first maximum in visiting order for allele subsets (mcall.c:583), the first of two
equal genotypes (strict `best_lk < lk`, mcall.c:806-836), and the higher base first among ALTs of equal QS (a stable
ascending sort walked from the top, bam2bcf.c:578-598)."""
import numpy as np
import pytest

from bcftools_amd import abi, host
from tests.helpers import orc
from tests.helpers import mcallgen as mg


def _values(cin):
    return cin.pl[(cin.pl != abi.INT32_MISSING) & (cin.pl != abi.INT32_VECTOR_END)]


@pytest.mark.parametrize("seed,n_smpl,use_ploidy,n_grp", [(1, 64, False, 1), (2, 257, True, 3), (3, 1001, True, 13)])
def test_cohort_records_reach_every_pl_range(seed, n_smpl, use_ploidy, n_grp):
    cin = mg.cohort_records(seed, 12, n_smpl, use_ploidy, n_grp, shuffled=True, use_prior=True)
    v = _values(cin)
    assert cin.n_gt_max == 15
    for e in mg.EDGE_PLS:
        assert (v == e).any(), e
    # depth 120 alone gives thousands, not only the explicit entries
    assert (v > 1000).sum() > 10 * len(mg.EDGE_PLS)
    assert ((v >= mg.PL_SUBNORMAL) & (v < mg.PL_ZERO)).sum() > 0 and (v >= mg.PL_ZERO).sum() > 0
    # 10^(-PL/10) as the oracle's libm gives it: subnormal from 3077, zero from 3237
    assert 0 < 10.0 ** (-mg.PL_SUBNORMAL / 10.0) < np.finfo(np.float64).tiny <= 10.0 ** (-(mg.PL_SUBNORMAL - 1) / 10.0)
    assert 10.0 ** (-mg.PL_ZERO / 10.0) == 0.0 < 10.0 ** (-(mg.PL_ZERO - 1) / 10.0)
    # every diploid sample without holes keeps a 0; a sample with a missing entry stays below 256 (outside: the table read
    # of mcall.c:522)
    for k in range(cin.n_sites):
        na = int(cin.nals[k])
        p = cin.pl[k, :na * (na + 1) // 2]
        ok = (p != abi.INT32_VECTOR_END) & (p != abi.INT32_MISSING)
        has = ok.any(axis=0)
        assert (p == 0).any(axis=0)[ok.all(axis=0)].all()
        holes = (p == abi.INT32_MISSING).any(axis=0) & has
        assert (np.where(ok, p, 0)[:, holes] < 256).all()
    assert (cin.pl == abi.INT32_MISSING).any() and cin.i16[:, :4].max() > 1000
    # the oracle calls variants on them: more than one allele kept at some sites
    cfg = abi.default_cfg(n_smpl, max_sites=cin.n_sites, n_grp=n_grp, output_tags=abi.CALL_FMT_GQ)
    want = orc.mcall(cfg, cin)
    assert (want.site["nals_new"] >= 2).sum() >= 3
    # and never the unseen allele (undefined behaviour in the reference: it writes past nals_new)
    us = cin.unseen > 0
    assert us.any() and not ((want.site["als_new"][us] >> cin.unseen[us]) & 1).any()


@pytest.mark.parametrize("use_ploidy,n_grp", [(False, 1), (True, 3)])
def test_tie_records_are_symmetric(use_ploidy, n_grp):
    cin, kinds = mg.tie_records(5, 120, use_ploidy=use_ploidy, n_grp=n_grp, shuffled=True)
    for k, kind in enumerate(kinds):
        na, _, _, (lo, hi), _ = mg.TIE_KINDS[kind]
        assert cin.qs[k, lo] == cin.qs[k, hi] > 0
        sym = mg.symmetric_samples(cin, k, lo, hi)
        assert sym.sum() > 0 if kind == "gt" else sym.all(), kind     # "gt": its 0/1 and 0/2 samples are not
        if n_grp > 1:
            for g in range(n_grp):
                a = cin.ad[k][:, cin.grp == g]
                assert a[lo].sum() == a[hi].sum()


@pytest.mark.parametrize("n_smpl,use_ploidy,n_grp", [(40, False, 1), (200, True, 1), (100, False, 3), (301, True, 13)])
def test_oracle_mcall_keeps_the_first_of_tied_alleles(n_smpl, use_ploidy, n_grp):
    cin, kinds = mg.tie_records(7 + n_smpl, n_smpl, use_ploidy=use_ploidy, n_grp=n_grp, shuffled=True)
    want = orc.mcall(abi.default_cfg(n_smpl, max_sites=cin.n_sites, n_grp=n_grp, output_tags=abi.CALL_FMT_GQ), cin)
    for k, kind in enumerate(kinds):
        lo, hi = mg.TIE_KINDS[kind][3]
        als = int(want.site["als_new"][k])
        if kind == "gt":
            assert als >> lo & 1 and als >> hi & 1
            sym = mg.symmetric_samples(cin, k, lo, hi)
            g = want.gt[k][:, sym]
            assert not mg.later_without_earlier(g, want.site["als_map"][k], lo, hi).any()
            assert (g == want.site["als_map"][k][lo]).sum() > n_smpl // 8
        else:
            assert als >> lo & 1 and not als >> hi & 1, (kind, bin(als))


@pytest.mark.parametrize("ref_n", [False, True])
def test_oracle_mpileup_orders_tied_alts_and_calls_the_first(ref_n):
    n_sites, S = 12, 150
    tile, lo, hi = mg.tie_tile(11, n_sites, S, ref_n=ref_n)
    cfg = abi.default_cfg(S, max_sites=n_sites, max_reads=len(tile.rd), fmt_flag=abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD)
    m = orc.mpileup(cfg, tile)
    na = m.site["n_alleles"]
    assert (na == (5 if ref_n else 4)).all()
    cin = host.CallInput(S, na, np.maximum(m.site["unseen"], 0), m.pl.astype(np.int32), m.site["qsum"])
    c = orc.mcall(cfg, cin)
    kinds = set()
    for k in range(n_sites):
        a = list(m.site["a"][k])
        j = a.index(hi[k])
        assert a[j + 1] == lo[k] and m.site["qsum"][k][j] == m.site["qsum"][k][j + 1] > 0
        np.testing.assert_array_equal(m.adf[k][j] + m.adr[k][j], m.adf[k][j + 1] + m.adr[k][j + 1])
        assert mg.symmetric_samples(cin, k, j, j + 1).all()          # PL planes mirror each other
        als = int(c.site["als_new"][k])
        assert als >> j & 1 or not als >> (j + 1) & 1
        assert not mg.later_without_earlier(c.gt[k], c.site["als_map"][k], j, j + 1).any()
        kinds.add((als >> j & 1, als >> (j + 1) & 1))
    assert (1, 0) in kinds and (1, 1) in kinds                       # a tied pair of subsets, and tied genotypes
