"""The inputs of tests/test_gpu_site_stats.py, checked on the CPU: the numpy twin of the site histograms against the full
oracle on every tile the GPU file uses, the oracle's Mann-Whitney density against an exact recursion, and the conditions
under which a deep tile can show a wrapped 16-bit counter at all."""
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import sitestats as ss

DEEP_STAT_CASES = ["A1", "A2", "two_wg_half", "slots"]
REGIME_SMPL = [3, 48]


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _check_twin(tile, want):
    tw = ss.twin_stats(tile)
    for k in ss.STATS:
        assert _bits_equal(tw[k], want.site[k]), (k, tw[k], want.site[k])
    # (SGB: the twin adds the terms with math.fsum, the oracle in sample order)
    sgb, w = tw["seg_bias"].astype(np.float64), want.site["seg_bias"].astype(np.float64)
    assert np.array_equal(np.isinf(sgb), np.isinf(w))
    np.testing.assert_allclose(w[~np.isinf(w)], sgb[~np.isinf(w)], rtol=ss.RTOL, atol=0, err_msg="seg_bias")
    np.testing.assert_array_equal(ss.twin_sp(tile), want.sp)
    np.testing.assert_array_equal(ss.cell_dp4(tile), want.dp4.astype(np.int64))


@pytest.mark.parametrize("name", sorted(ss.DEEP_CASES))
def test_twin_equals_oracle_on_deep_tiles(name):
    """The five float site fields and FMT/SP of the twin are the full oracle's to the last bit of float32, DP4 too."""
    tile, cfg, want = ss.deep_case(name)
    assert len(tile.rd) < 600000
    _check_twin(tile, want)


@pytest.mark.parametrize("name", DEEP_STAT_CASES)
def test_deep_tiles_have_finite_statistics(name):
    """On four deep tiles every one of the five statistics is a finite number at some site (not the 'no ALT read' answer)."""
    tile, cfg, want = ss.deep_case(name)
    for k in ss.STATS:
        assert np.isfinite(want.site[k]).any(), k


# ---------------------------------------------------------------------------------------------------------------------
# exact Mann-Whitney
# ---------------------------------------------------------------------------------------------------------------------
def _arrangements(na, nb, U):
    """The number of orders of na a's and nb b's (no ties) in which sum over a of (b's before it) is U.  Python integers."""
    cnt = {}

    def N(n, m, u):
        if u < 0:
            return 0
        if n == 0 or m == 0:
            return 1 if u == 0 else 0
        key = (n, m, u)
        if key not in cnt:
            cnt[key] = N(n - 1, m, u - m) + N(n, m - 1, u)       # the last element is an a (after all m b's), or a b
        return cnt[key]
    return N(na, nb, U)


def _hists_with_U(na, nb):
    """{U: (a, b)}: for every integer U in 0..na*nb an order of na a's and nb b's, a bin per read, with that statistic; and for
    every half-integer U the same order with one adjacent (b, a) pair put in one bin (a tie: 1/2 instead of 1)."""
    out = {}
    for where in itertools.combinations(range(na + nb), na):
        is_a = np.zeros(na + nb, bool)
        is_a[list(where)] = True
        U = int((np.cumsum(~is_a)[is_a]).sum())
        if U not in out:
            out[U] = (is_a.astype(np.int32), (~is_a).astype(np.int32))
            tie = [i for i in range(na + nb - 1) if not is_a[i] and is_a[i + 1]]
            if tie:
                i = tie[0]
                a, b = is_a.astype(np.int32), (~is_a).astype(np.int32)
                a[i] = 1
                a[i + 1] = b[i + 1] = 0
                out[U - 0.5] = (a, b)
        if len(out) == 2 * na * nb + 1:
            break
    return out


def test_mwu_density_matches_exact_recursion():
    """calc_mwu_bias for 3 <= na, nb <= 7 is (arrangements with statistic U) / C(na+nb, na) * sqrt(2 pi var), with U cut to an
    integer (bam2bcf.c:483 passes the double U to an int parameter).  Every reachable integer and half-integer U, both
    orders of (na, nb), the corners U = 0 and U = na*nb.  The exact value is formed with Python integers and fractions and
    rounded once.  Largest relative deviation measured over the whole domain: 5.9e-16 (the oracle fills its table with the
    recursion in doubles; the reference's printed table has more digits than a double keeps), hence the bound 1e-15."""
    worst = 0.0
    seen = 0
    for na in range(3, 8):
        for nb in range(3, 8):
            hs = _hists_with_U(na, nb)
            assert sorted(hs) == [x / 2 for x in range(2 * na * nb + 1)]
            var2 = Fraction(na * nb * (na + nb + 1), 12)
            for U, (a, b) in hs.items():
                dens = Fraction(_arrangements(na, nb, int(U)), math.comb(na + nb, na))
                want = float(dens) * math.sqrt(2 * math.pi * float(var2))
                got = ss.mwu(np.r_[a, np.zeros(60 - len(a), np.int32)], np.r_[b, np.zeros(60 - len(b), np.int32)])
                assert want > 0
                worst = max(worst, abs(got - want) / want)
                seen += 1
    print("largest relative deviation over %d points: %.3g" % (seen, worst))
    assert worst <= 1e-15


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity conditions of part A
# ---------------------------------------------------------------------------------------------------------------------
def _detectable(tile, own):
    """The statistics whose true value differs, at some site, from the one wrapped counters would give by more than 100 x
    the comparison tolerance."""
    out = set()
    for s in range(tile.n_sites):
        true, wrap = ss.stats_of(ss.site_hists(tile, s)), ss.stats_of(ss.wrapped_site_hists(tile, s, own))
        out |= {k for k in ss.STATS if ss.differs(true[k], wrap[k])}
    return out


@pytest.mark.parametrize("name", sorted(ss.DEEP_CASES))
def test_deep_case_claims_hold(name):
    case = ss.DEEP_CASES[name]
    tile, cfg, want = ss.deep_case(name)
    det = _detectable(tile, case.own)
    print(name, "detectable:", sorted(det))
    # (a statistic that underflows to 0 with and without the wrap is not detectable: differs() is false for it)
    assert set(case.claims) <= det, (name, sorted(det))
    for s in range(tile.n_sites):
        h = ss.site_hists(tile, s)
        # where b[i] == 0 the reference forms a[i] * nb as an int: below 2^31 at every site and for every histogram pair
        for a, b in (("ref_pos", "alt_pos"), ("ref_mq", "alt_mq"), ("ref_bq", "alt_bq"), ("fwd_mqs", "rev_mqs")):
            assert ss.mwu_int_products_ok(h[a], h[b]), (name, s, a)
    # no cell has more than 65 535 reads of one base and strand
    assert ss.cell_dp4(tile).max() <= 65535


def test_every_statistic_is_claimed_in_both_single_site_groups():
    for group in ("one_wg", "two_wg"):
        claimed = set()
        for c in ss.DEEP_CASES.values():
            if c.group == group:
                claimed |= set(c.claims)
        assert claimed == set(ss.STATS), (group, sorted(claimed))


def test_case_shapes():
    """What the cases are for: a bin past 65 535 in the form they name."""
    a3 = ss.site_hists(ss.deep_case("A3")[0], 0)
    assert a3["ref_bq"][40] == 65535 and a3["ref_pos"][50] == 65536 and a3["ref_mq"][40] == 65536 and a3["fwd_mqs"][40] == 65536
    for name in ("A1", "A2", "two_wg_half", "two_wg_alt3", "two_wg_few_alt", "slots", "listed", "A1_indel", "A2_indel", "spread_indel"):
        tile, case = ss.deep_case(name)[0], ss.DEEP_CASES[name]
        assert tile.n_smpl >= 37                              # the packed form
        over = 0
        for s in range(tile.n_sites):
            for a, b in ss.workgroup_pieces(tile, s, case.own):
                h = ss.cell_range_hists(tile, s, a, b)
                over += sum(int((h[k] > 65535).sum()) for k in ss.HISTS)
        assert over > 0, name
    a2 = ss.site_hists(ss.deep_case("A2")[0], 0)
    assert a2["ref_pos"][50] > 65535 and a2["alt_pos"][50] > 65535 and a2["fwd_mqs"][59] > 65535 and a2["rev_mqs"][59] > 65535
    assert ss.deep_case("control")[0].n_smpl == 36 and ss.deep_case("slots")[0].n_smpl == 37
    tile = ss.deep_case("listed")[0]
    d = ss.cell_dp4(tile)[0, :, ss.LISTED_CELL]
    assert d[0] == 40000 and d[1] == 40000 and d[2] + d[3] == 3000
    two = ss.deep_case("two_wg_half")[0]
    assert [b - a for a, b in ss.workgroup_pieces(two, 0)] == [256, 44]


def test_wrapped16():
    lo, hi = ss.wrapped16([65535, 65536, 70000, 3], [1, 1, 65535, 65536])
    assert lo.tolist() == [65535, 0, 70000 - 65536, 3] and hi.tolist() == [1, 2, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# part B: the regime tiles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_smpl", REGIME_SMPL + [0])
def test_twin_equals_oracle_on_regime_tiles(n_smpl):
    tile, cfg, want = ss.regime_case(n_smpl)
    _check_twin(tile, want)


@pytest.mark.parametrize("n_smpl", REGIME_SMPL)
def test_regime_tile_meets_every_regime(n_smpl):
    """Every branch of calc_mwu_bias (for each of RPB, MQB, BQB and MQSB), of calc_vdb and of FMT/SP occurs in the tile."""
    tile, cfg, want = ss.regime_case(n_smpl)
    seen = ss.regimes(tile)
    print({k: sorted(v) for k, v in seen.items()})
    ss.assert_regime_coverage(tile)
    assert (want.sp == 255).any() and (want.sp == 0).any()


def test_replay_tile_passes_2_24():
    tile, cfg, want = ss.regime_case(0)
    h = ss.site_hists(tile, 0)
    assert "replay" in ss.vdb_regimes(h["alt_pos"])
    assert max(int(h[k].max()) for k in ss.HISTS) < 1 << 14 and np.isfinite(want.site["vdb"][0]) and want.site["vdb"][0] > 0
