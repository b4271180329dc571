"""The inputs of tests/test_gpu_i16.py, checked on the CPU: the regimes the I16 vectors have to reach, what the oracle makes of
them (DP4, MQ, whether a site is tested, exact zeros, NaN), and the oracle's test16 itself against exact rationals (Fisher)
and against mpmath's incomplete beta function at 40 digits (the t-tests)."""
from fractions import Fraction

import numpy as np
import pytest

from bcftools_amd import abi
from tests.helpers import i16stats as i16

SITE_COUNTS = [0, 1, 15, 16, 17, 33]           # 0: the whole catalog


def test_catalog_meets_every_regime():
    vecs = [v for _, v in i16.catalog()]
    print(sorted(i16.seen(vecs)))
    i16.assert_coverage(vecs)
    # every t-test regime in every one of the three statistics
    for k in i16.T_NEED:
        assert {"%s_%s" % (k, nm) for nm in i16.STATS} <= i16.PV4_NEED
    # the longest continued fraction: t near 1.7 at v >= 1000
    steps = []
    for name, v in i16.catalog():
        if name.startswith(("long_", "v58000_")):
            k = i16.STATS.index(name.rsplit("_", 1)[1])
            n1, n2 = int(v[0] + v[1]), int(v[2] + v[3])
            kind, t, dof, x = i16.ttest_parts(n1, n2, v[4 + 4 * k:8 + 4 * k])
            sw = (dof / 2 + 1) / (dof / 2 + 2.5)
            steps.append(i16.betai_steps(dof / 2, .5, x) if x < sw else i16.betai_steps(.5, dof / 2, 1 - x))
    print("continued-fraction terms near the switch:", sorted(set(steps)))
    assert max(steps) >= 70 and max(steps) < 199


def test_nan_search():
    """Constant-quality sites of 9000..30000 REF and 3000..9000 ALT reads, ALT one quality below REF: the float32 sums of squares
    are past 2^24, the variance rounds below 0 and the oracle's p is NaN.  About one draw in six qualifies."""
    found = i16.nan_search()
    assert len(found) == 3
    for n1, n2, Q in found:
        a4 = i16.moments(np.full(n1, Q), np.full(n2, Q - 1))
        assert max(a4) > 1 << 24
        for k in range(3):
            v = i16.vector(i16.split(n1, n2), [a4 if j == k else i16.filler(n1, n2, j) for j in range(3)])
            rc, p, tested = i16.oracle_test16(v)
            assert rc == 0 and tested and np.isnan(p[1 + k]) and not np.isnan(np.delete(p, 1 + k)).any()


@pytest.mark.parametrize("n_sites", SITE_COUNTS)
def test_arrangements(n_sites):
    """Special sites on either side of every boundary between two workgroups of sixteen sites and at the end; skipped records
    between the called ones, never at a special place; the oracle leaves a skipped record's I16 fields unset."""
    names, cin, skipped, cfg, want = i16.mcall_case(n_sites)
    n = len(names)
    assert n == n_sites or not n_sites and n > len(i16.catalog())
    assert np.array_equal(skipped, [k.startswith("skip:") for k in names])
    for i in range(1, n):
        if i % i16.WG_SITES in (0, i16.WG_SITES - 1):
            assert names[i] in i16.SPECIAL and not skipped[i], i
    assert names[-1] in i16.SPECIAL
    st = want.site
    assert np.array_equal(st["ret"] <= 0, skipped) and (st["ret"][~skipped] == 2).all() and (st["nals_new"][skipped] == 0).all()
    assert skipped.any() == (n > 2)
    for k in ("has_i16", "pv4_tested", "mq"):
        assert (st[k][skipped] == 0).all()
    assert (st["dp4"][skipped] == 0).all() and (st["pv4"][skipped] == 0).all() and (st["has_i16"][~skipped] == 1).all()
    if n_sites == 0:
        # every vector of the catalog on a called record
        assert {k for k, _ in i16.catalog()} == {k for k in names if not k.startswith("skip:")}
        i16.assert_coverage(cin.i16[~skipped])


def _site(want, names, name):
    return want.site[names.index(name)]


def test_what_the_oracle_makes_of_the_regimes():
    names, cin, skipped, cfg, want = i16.mcall_case(0)
    s = lambda k: _site(want, names, k)
    d0 = s("depth_0")
    assert d0["has_i16"] == 1 and d0["mq"] == abi.INT32_MISSING and d0["pv4_tested"] == 0 and (d0["dp4"] == 0).all() and (d0["pv4"] == 0).all()
    r, a = s("ref_only"), s("alt_only")
    assert r["dp4"].tolist() == [5, 6, 0, 0] and r["mq"] == 40 and r["pv4_tested"] == 0 and (r["pv4"] == 0).all()
    assert a["dp4"].tolist() == [0, 0, 4, 3] and a["mq"] == 40 and a["pv4_tested"] == 0 and (a["pv4"] == 0).all()
    assert [int(s(k)["mq"]) for k in ("mq_below", "mq_on", "mq_above")] == [39, 40, 40]
    # 17 400 029 / 600 001 is 29; the float sum is 17 400 028 and the float quotient below 29
    assert s("sum_rounds")["mq"] == 28 and s("sum_rounds")["dp4"].tolist() == [300000, 300000, 1, 0]
    assert Fraction(17400029, 600001) == 29 and np.float32(17400000) + np.float32(29) == 17400028
    for k, nm in enumerate(i16.STATS):
        p = s("zero_var_" + nm)["pv4"]
        assert p[1 + k] == 0 and (np.delete(p, 1 + k) > 0).all()
        p = s("neg_var_" + nm)["pv4"]
        assert np.isnan(p[1 + k]) and not np.isnan(np.delete(p, 1 + k)).any()
        p = s("p_subnormal_" + nm)["pv4"]
        assert 0 < p[1 + k] < i16.F32_MIN_NORMAL
        assert s("p_float_zero_" + nm)["pv4"][1 + k] == 0
        for nn in ("n_lt3_", "means_equal_", "alt_higher_"):
            assert s(nn + nm)["pv4"][1 + k] == 1
    assert s("fisher_10000_0_0_10000")["pv4"][0] == 0 and s("fisher_10000_0_0_10000")["pv4_tested"] == 1
    for k in ("fisher_1_1_1_1", "fisher_2_2_2_2", "fisher_5_0_7_0", "fisher_0_6_0_3", "fisher_7500_7500_7500_7500"):
        assert s(k)["pv4"][0] == 1
    assert 0 < s("fisher_8000_7000_7000_8000")["pv4"][0] < 1e-20


def test_pv4_tag_off():
    names, cin, skipped, cfg, want = i16.mcall_case(0, 0)
    on = i16.mcall_case(0)[4]
    assert (want.site["pv4_tested"] == 0).all() and (want.site["pv4"] == 0).all()
    for k in ("has_i16", "dp4", "mq", "ret"):
        np.testing.assert_array_equal(want.site[k], on.site[k])
    assert (want.site["dp4"].sum(axis=1) > 0).sum() > 40


def test_fused_sites():
    """The sites built from reads: the mpileup stage's I16, cast to float, are the intended vectors exactly; the deep
    constant-quality site gives NaN and the zero-variance site exact zeros, next to each other across a workgroup boundary."""
    names, tile, vecs, cfg, mwant, cwant = i16.fused_case()
    assert tile.n_sites == 17 and names[15:] == ["neg_var", "zero_var"] and len(tile.rd) < 45000
    np.testing.assert_array_equal(mwant.site["anno"].astype(np.float32), vecs)
    i16.assert_coverage(vecs, i16.FUSED_NEED)
    st = cwant.site
    live = st["ret"] > 0
    assert live[15] and live[16] and (~live).sum() >= 3 and not live[[names.index("ref_only")]].any()
    assert np.isnan(st["pv4"][15, 1]) and st["pv4_tested"][15] == 1
    assert st["pv4"][16].tolist() == [1, 0, 0, 0] and st["pv4_tested"][16] == 1
    assert st["pv4_tested"][names.index("alt_only")] == 0 and st["has_i16"][names.index("alt_only")] == 1
    assert (st["has_i16"][~live] == 0).all()


def test_comparison_rule():
    """assert_pv4_close: no absolute term; NaN only against NaN, 0 only against 0, one subnormal step below the normal range."""
    f = lambda *x: np.array(x, np.float32)
    i16.assert_pv4_close(f(1, 0, np.nan, 1e-40, 1e-20), f(1, 0, np.nan, 1e-40 + 1.4e-45, 1e-20 * (1 + 1e-6)))
    for got, want in ((f(0), f(1e-45)), (f(1e-45), f(0)), (f(np.nan), f(1)), (f(1), f(np.nan)), (f(1e-31), f(2e-31)),
                      (f(1e-40), f(1.1e-40)), (f(1.00001), f(1)), (f(1e-20), f(1.00001e-20))):
        with pytest.raises(AssertionError):
            i16.assert_pv4_close(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's test16 against exact and high-precision references
# ---------------------------------------------------------------------------------------------------------------------
FISHER_BOUND = 1.92e-9
TTEST_BOUND = 2.46e-8


def test_fisher_against_exact_rationals():
    """orc_test16's p[0] against kt_fisher_exact's rule in exact rational arithmetic (math.comb, fractions), clamped at 1, over
    every table of the catalog of at most 40 000 reads and every table of sitestats.SP_TABLES, where the exact value is a
    double above 1e-300.  Largest relative deviation measured over the 31 tables: 1.92e-11 (at (8000, 7000, 7000, 8000): the
    terms come from differences of kf_lgamma values near 1e5); the bound is 100 x that, 1.92e-9, a thousandth of the device
    tolerance."""
    from tests.helpers import sitestats as ss
    tables = {tuple(int(x) for x in v[:4]) for _, v in i16.catalog()} | set(ss.SP_TABLES)
    worst, at, n = 0.0, None, 0
    for t in sorted(tables):
        if not (t[0] + t[1] and t[2] + t[3]) or sum(t) > 40000:
            continue
        v = np.zeros(16, np.float32)
        v[:4] = t
        got = i16.oracle_test16(v)[1][0]
        two, own = i16.fisher_kfunc_exact(*t)
        want = float(min(two, 1))
        if want < 1e-300:
            assert got == 0 or got < 1e-290
            continue
        dev = abs(got - want) / want
        n += 1
        if dev > worst:
            worst, at = dev, t
    print("largest relative deviation over %d tables: %.3g at %s" % (n, worst, at))
    assert n >= 30 and worst <= FISHER_BOUND
    assert FISHER_BOUND <= i16.RTOL / 10


def test_ttest_against_mpmath():
    """orc_test16's t-test p-values against 1/2 I_x(v/2, 1/2) from mpmath.betainc at 40 digits, t and x formed at that precision
    from the float32 inputs, over every block of the catalog and of the sites built from reads whose p is finite and not 0
    (down to 1e-128).  Largest relative deviation measured over the 166 values: 2.46e-10 (at v = 58 000: the three kf_lgamma
    values are near 3e5 and their difference loses six digits); the bound is 100 x that, 2.46e-8, an 80th of the device
    tolerance."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    vecs = [v for _, v in i16.catalog()] + list(i16.fused_case()[2])
    worst, at, n = 0.0, None, 0
    for v in vecs:
        n1, n2 = int(v[0] + v[1]), int(v[2] + v[3])
        if not n1 or not n2:
            continue
        got = i16.oracle_test16(v)[1]
        for k in range(3):
            a = v[4 + 4 * k:8 + 4 * k]
            if i16.ttest_parts(n1, n2, a)[0] != "beta":
                continue
            a = [mp.mpf(float(x)) for x in a]
            u1, u2 = a[0] / n1, a[2] / n2
            var = ((a[1] - n1 * u1 * u1) + (a[3] - n2 * u2 * u2)) / (n1 + n2 - 2) * (mp.mpf(1) / n1 + mp.mpf(1) / n2)
            dof = n1 + n2 - 2
            x = dof / (dof + (u1 - u2) ** 2 / var)
            want = mp.betainc(mp.mpf(dof) / 2, mp.mpf(1) / 2, 0, x, regularized=True) / 2
            assert want > 0 and got[1 + k] > 0
            dev = float(abs(mp.mpf(float(got[1 + k])) - want) / want)
            n += 1
            if dev > worst:
                worst, at = dev, (n1, n2, [float(y) for y in a])
    print("largest relative deviation over %d p-values: %.3g at %s" % (n, worst, at))
    assert n >= 100 and worst <= TTEST_BOUND
    assert TTEST_BOUND <= i16.RTOL / 10
