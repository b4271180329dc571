"""The inputs of tests/test_gpu_sgb.py, checked on the CPU: the oracle's calc_SegBias against the math.fsum twin on every
tile, the regimes each tile has to reach, the conditioning of the sum, and the proof that each tile could show the mistakes
that combine_kernel's way of summing SGB invites."""
import math

import numpy as np
import pytest

from tests.helpers import sgbstats as sg
from tests.helpers import sitestats as ss

FORMS = [False, True]


def _assert_twin(tile, want):
    tw = ss.twin_seg_bias(tile).astype(np.float64)
    w = want.site["seg_bias"].astype(np.float64)
    assert np.array_equal(np.isinf(tw), np.isinf(w)) and not np.isnan(w).any()
    m = ~np.isinf(w)
    np.testing.assert_allclose(w[m], tw[m], rtol=ss.RTOL, atol=0)
    return m


@pytest.mark.parametrize("indel", FORMS)
@pytest.mark.parametrize("n_smpl", sg.SAMPLE_COUNTS)
def test_oracle_equals_twin(n_smpl, indel):
    tile, cfg, want = sg.sgb_case(n_smpl, indel)
    assert tile.n_smpl == n_smpl and len(tile.rd) < 300000
    fin = _assert_twin(tile, want)
    d = ss.cell_dp4(tile)
    no_alt = (d[:, 2] + d[:, 3]).sum(axis=1) == 0
    assert no_alt.sum() >= 2 and 0 < np.nonzero(no_alt)[0].max() < tile.n_sites - 1      # one of them between live sites
    if indel:
        # no read of an indel type: the record is dropped, every field of the site is 0 (not +inf)
        assert (want.site["ret"][no_alt] == -1).all() and (want.site["seg_bias"][no_alt] == 0).all() and fin.all()
        assert (want.site["ret"][~no_alt] == 0).all()
    else:
        assert np.array_equal(~fin, no_alt)                  # +inf, the tag omitted, exactly where there is no ALT read
    # the planes hold the deep cell's two counts, and their sum is past 16 bits
    s = int(np.argmax(d[:, 2].max(axis=1)))
    assert want.dp4[s, 2, sg.DEEP_AT[n_smpl]] == sg.DEEP_FWD and want.dp4[s, 3, sg.DEEP_AT[n_smpl]] == sg.DEEP_REV


@pytest.mark.parametrize("name", sorted(ss.DEEP_CASES))
def test_oracle_equals_twin_on_deep_tiles(name):
    tile, cfg, want = ss.deep_case(name)
    _assert_twin(tile, want)


@pytest.mark.parametrize("n_smpl", [3, 48, 0])
def test_oracle_equals_twin_on_regime_tiles(n_smpl):
    tile, cfg, want = ss.regime_case(n_smpl)
    _assert_twin(tile, want)


@pytest.mark.parametrize("n_smpl", sg.SAMPLE_COUNTS)
def test_tile_meets_every_regime(n_smpl):
    tile = sg.sgb_case(n_smpl)[0]
    print(sorted(sg.seen_regimes(tile)))
    sg.assert_sgb_coverage(tile)
    assert sg.seen_regimes(sg.sgb_case(n_smpl, True)[0]) == sg.seen_regimes(tile)
    worst = sg.assert_kappa(tile)
    print("largest condition number: %.3g" % worst)


def test_need_sets():
    """What a tile has to reach: everything, but for what one sample cannot; 511 and 512 at every chosen place the sample count
    has; and the deep cell at every chosen place in some tile."""
    assert sg.SGB_NEED <= sg.sgb_need(3) and sg.sgb_need(1) & sg.ONE_SAMPLE_CANNOT == set()
    assert {"oi_%d_at_%s" % (v, p) for v in (511, 512) for p in ("first", "last", "s63", "s64", "s255", "s256")} <= sg.sgb_need(257)
    deep = set()
    for S in sg.SAMPLE_COUNTS:
        deep |= {k for k in sg.sgb_need(S) if k.startswith("deep_at_")}
    assert deep == {"deep_at_" + p for p in ("first", "last", "s63", "s64", "s255", "s256")}
    # the sample counts: one lane per sample with a second round of 64 and of 256 (65, 257), four per lane with one (260)
    assert [S % 4 == 0 for S in sg.SAMPLE_COUNTS] == [False, False, True, False, True, False, True]


# One sample: M = n = 1, so f = 1/2 and q = p = nr = oi, and the sample's term is log(1/2) + log(1 + 2^(oi-1) e^(-oi)): from
# oi = 40 it is log(1/2) to the last bit whatever oi is taken to be.  Only leaving the term out can show there.
BLIND_AT_ONE_SAMPLE = {"b_clipped_511", "b_clipped_255", "c_sum_in_16_bits"}


@pytest.mark.parametrize("indel", FORMS)
@pytest.mark.parametrize("n_smpl", sg.SAMPLE_COUNTS)
def test_tile_could_show_each_mistake(n_smpl, indel):
    """The twin recomputed under a model of each mistake differs at some site by more than 100 x the comparison's tolerance
    (or is no number at all): cells from 512 ALT reads left out, the count clipped to 511 or to 255 or formed in 16 bits, the
    samples from 256 on or the last n_smpl % 4 left out, M without its upper or without its lower clamp."""
    tile = sg.sgb_case(n_smpl, indel)[0]
    c = sg.caught(tile)
    print({k: v for k, v in c.items()})
    want = {"a_deep_left_out", "b_clipped_511", "b_clipped_255", "c_sum_in_16_bits", "f_M_0_kept"}
    if n_smpl > 256:
        want.add("d_second_round_left_out")
    if n_smpl % 4:
        want.add("e_ragged_tail_left_out")
    if n_smpl > 1:
        want.add("f_M_above_n_kept")
    assert set(c) == want
    for k in want - (BLIND_AT_ONE_SAMPLE if n_smpl == 1 else set()):
        assert c[k], k


def test_twin_formula():
    """The twin against the formula written out for cases small enough to do by hand."""
    # one sample, one ALT read of two reads: avg_dp = 2, M = floor(1) = 1, f = 1/2, p = q = 1
    v, kappa = ss.sgb_twin([1, 0, 1, 0], [1], 1)
    assert v == pytest.approx(math.log(1 + math.exp(math.log(.5) + math.log(2) - 1)) + math.log(.5), rel=1e-15) and kappa == pytest.approx(1)
    # two samples, reads (2 REF | 2 ALT): avg_dp = 2, M = 1, f = 1/4, p = 1, q = 2
    f, p, q = .25, 1., 2.
    t0 = math.log(2 * f * (1 - f) * math.exp(-q) + f * f * math.exp(-2 * q) + (1 - f) ** 2) + p
    a, b = math.log(2 * (1 - f)), math.log(f) + 2 * math.log(2) - q
    t1 = math.log(1 + math.exp(b - a)) + a + math.log(f) + 2 * math.log(q / p) - q + p
    assert ss.sgb_twin([2, 0, 1, 1], [0, 2], 2)[0] == pytest.approx(t0 + t1, rel=1e-15)
    assert ss.sgb_twin([5, 5, 0, 0], [0, 0], 2)[0] == math.inf
    # fewer reads than samples: the division by avg_dp = 0 gives M = n
    f, p, q = .5, 1 / 3, 1 / 3
    t0 = math.log(2 * f * (1 - f) * math.exp(-q) + f * f * math.exp(-2 * q) + (1 - f) ** 2) + p
    b = math.log(f) + math.log(2) - q                        # (below log(2 * (1 - f)) = 0)
    t1 = math.log(1 + math.exp(b)) + math.log(f) - q + p
    assert ss.sgb_twin([0, 0, 1, 0], [1, 0, 0], 3)[0] == pytest.approx(t1 + 2 * t0, rel=1e-15)
    assert math.isnan(ss.sgb_twin([0, 0, 1, 0], [1, 0, 0], 3, clamp_hi=False)[0])
