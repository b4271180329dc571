"""Directed inputs for INFO/SGB (calc_SegBias, bam2bcf.c:494-530; combine_kernel's pass over the DP4 planes).

The twin is sitestats.sgb_twin.  A tile is a list of sites given as per-sample (REF, ALT) read counts; `sgb_regimes`
names the branches of the formula and of the kernel's way of summing it that a site reaches (samples by ALT depth 0,
1..511 and from 512; rounds of 256 samples; the tail of a sample count that is no multiple of 4), and `sgb_need` lists
what a tile of a given sample count has to reach.  `sgb_mutants` recomputes the twin under models of the mistakes that
this way of summing invites; tests/test_oracle_sgb.py asserts that each moves SGB of some site of each tile.
"""
import functools
import math

import numpy as np

from . import orc
from . import sitestats as ss

SAMPLE_COUNTS = (1, 3, 4, 65, 256, 257, 260)
OI_VALUES = (0, 1, 255, 256, 511, 512, 513)
DEEP_FWD, DEEP_REV = 40000, 30000                  # one cell's ALT reads: either plane holds it, their sum is past 65 535
Q_LARGE = 800                                      # exp(-q) and exp(-2q) are 0 from q = 746
KAPPA_MAX = 1e3
# the sample that holds the tile's deep cell: between the tiles, every one of the chosen places
DEEP_AT = {1: 0, 3: 2, 4: 0, 65: 63, 256: 255, 257: 256, 260: 64}


def places(n_smpl):
    """{name: sample} of the chosen places: the first and the last sample, either side of a wavefront's 64 lanes and of a
    round's 256 samples."""
    p = {"first": 0, "last": n_smpl - 1, "s63": 63, "s64": 64, "s255": 255, "s256": 256}
    return {k: v for k, v in p.items() if v < n_smpl}


# ---------------------------------------------------------------------------------------------------------------------
# regimes
# ---------------------------------------------------------------------------------------------------------------------
def sgb_regimes(d):
    """The regimes one site reaches; d: its cells' DP4, int [4][n_smpl] (a site of sitestats.cell_dp4)."""
    d = np.asarray(d, np.int64)
    S = d.shape[1]
    anno = d.sum(axis=1)
    oi = d[2] + d[3]
    nr = int(anno[2] + anno[3])
    if not nr:
        return {"no_alt"}
    out = set()
    avg_dp = int(anno.sum()) // S
    if avg_dp == 0:
        out.add("avg_dp_0")
        M = S
    else:
        x = nr / avg_dp
        M0 = math.floor(x + 0.5)
        if (2 * nr) % avg_dp == 0 and (2 * nr // avg_dp) % 2 == 1:
            out.add("M_half")
        if M0 == 0:
            out.add("M_0_to_1")
        elif M0 > S:
            out.add("M_clamped")
        elif M0 == 1:
            out.add("M_round_1")
        elif M0 == S:
            out.add("M_round_n")
        else:
            out.add("M_inside")
        M = min(max(M0, 1), S)
    if M == 1 and nr >= Q_LARGE and (oi == 0).any():
        out.add("q_large")
    out |= {"oi_%d" % v for v in OI_VALUES if (oi == v).any()}
    deep = (oi > 65535) & (d[2] <= 65535) & (d[3] <= 65535)
    if deep.any():
        out.add("oi_past_u16")
    if S > 1 and oi[0] > 0 and (oi == oi[0]).all():
        out.add("all_same")
    if S > 1 and len(set(oi.tolist())) == S:
        out.add("all_differ")
    for name, s in places(S).items():
        out |= {"oi_%d_at_%s" % (v, name) for v in (511, 512) if oi[s] == v}
        if deep[s]:
            out.add("deep_at_" + name)
    return out


SGB_NEED = ({"no_alt", "avg_dp_0", "M_0_to_1", "M_round_1", "M_inside", "M_round_n", "M_clamped", "M_half", "q_large",
             "oi_past_u16", "all_same", "all_differ"} | {"oi_%d" % v for v in OI_VALUES})
# One sample: nr / avg_dp is at most 1 and M is 1 whatever is clamped; a site with an ALT read has no sample without one.
ONE_SAMPLE_CANNOT = {"avg_dp_0", "M_inside", "M_round_n", "M_clamped", "q_large", "oi_0", "all_same", "all_differ"}


def sgb_need(n_smpl):
    need = SGB_NEED - ONE_SAMPLE_CANNOT if n_smpl == 1 else set(SGB_NEED)
    need |= {"oi_%d_at_%s" % (v, name) for v in (511, 512) for name in places(n_smpl)}
    need |= {"deep_at_" + name for name, s in places(n_smpl).items() if s == DEEP_AT[n_smpl]}
    return need


def seen_regimes(tile):
    d = ss.cell_dp4(tile)
    seen = set()
    for s in range(tile.n_sites):
        seen |= sgb_regimes(d[s])
    return seen


def assert_sgb_coverage(tile):
    seen, need = seen_regimes(tile), sgb_need(tile.n_smpl)
    assert need <= seen, sorted(need - seen)


def assert_kappa(tile):
    """The sum is well conditioned at every site: with kappa <= 1e3 and at most 1100 terms, adding the doubles in another
    order moves it by less than 1100 * 2^-53 * 1e3 = 1.3e-10 of its value, far below the comparison's 2e-6."""
    d = ss.cell_dp4(tile)
    worst = 0.0
    for s in range(tile.n_sites):
        anno = d[s].sum(axis=1)
        if anno[2] + anno[3]:
            v, kappa = ss.sgb_twin(anno, d[s, 2] + d[s, 3], tile.n_smpl)
            assert math.isfinite(v) and kappa <= KAPPA_MAX, (s, v, kappa)
            worst = max(worst, kappa)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# models of mistakes
# ---------------------------------------------------------------------------------------------------------------------
def sgb_mutants(anno, oi, n_smpl):
    """{model: SGB of the site under it}.  The site totals (nr, avg_dp) stay the true ones: the kernel has them from another
    pass.  A model that cannot apply at this sample count is absent."""
    oi = [int(x) for x in oi]
    S = n_smpl
    tw = lambda o, **kw: ss.sgb_twin(anno, o, S, **kw)[0]
    m = {
        "a_deep_left_out": tw([None if x >= 512 else x for x in oi]),
        "b_clipped_511": tw([min(x, 511) for x in oi]),
        "b_clipped_255": tw([min(x, 255) for x in oi]),
        "c_sum_in_16_bits": tw([x & 0xffff for x in oi]),
        "f_M_0_kept": tw(oi, clamp_lo=False),
    }
    if S > 256:
        m["d_second_round_left_out"] = tw(oi[:256] + [None] * (S - 256))
    if S % 4:
        m["e_ragged_tail_left_out"] = tw(oi[:S - S % 4] + [None] * (S % 4))
    if S > 1:
        m["f_M_above_n_kept"] = tw(oi, clamp_hi=False)
    return m


def moved(true, model):
    """The model's value is not the true one: not a number at all (M without a clamp gives log of a negative number), or
    further off than 100 x the comparison's tolerance."""
    return math.isnan(model) or ss.differs(true, model)


def caught(tile):
    """{model: the sites whose SGB it moves}."""
    d = ss.cell_dp4(tile)
    out = {}
    for s in range(tile.n_sites):
        anno, oi = d[s].sum(axis=1), d[s, 2] + d[s, 3]
        if not (anno[2] + anno[3]):
            continue
        true = ss.sgb_twin(anno, oi, tile.n_smpl)[0]
        for k, v in sgb_mutants(anno, oi, tile.n_smpl).items():
            out.setdefault(k, [])
            if moved(true, v):
                out[k].append(s)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------
def _site(rng, ref, alt, alt_rev=None):
    """Reads of one site from per-sample counts of REF and ALT reads (alt_rev: how many of a sample's ALT reads are on the
    reverse strand; random otherwise).  Qualities and positions from sitestats.LEVELS: every read is an accepted one."""
    ref, alt = np.asarray(ref, np.int64), np.asarray(alt, np.int64)
    S = len(ref)
    smpl = np.concatenate([np.repeat(np.arange(S), ref), np.repeat(np.arange(S), alt)]).astype(np.int64)
    is_alt = np.arange(len(smpl)) >= int(ref.sum())
    rev = rng.integers(0, 2, len(smpl))
    if alt_rev is not None:
        rev[is_alt] = np.concatenate([np.arange(a) < r for a, r in zip(alt, alt_rev)] + [np.zeros(0, bool)])
    lv = lambda k: rng.choice(ss.LEVELS[k], len(smpl)).astype(np.int64)
    return dict(smpl=smpl, alt=is_alt, rev=rev.astype(np.int64), bq=lv("bq"), mq=lv("mq"), epos=lv("epos"))


def _spread(total, S, skip=()):
    """`total` reads dealt as evenly as they go over the samples not in `skip`."""
    idx = [i for i in range(S) if i not in skip]
    out = np.zeros(S, np.int64)
    if idx:
        out[idx] = total // len(idx)
        out[idx[:total % len(idx)]] += 1
    return out


def site_counts(S, seed):
    """The sites of a tile of S samples as (REF counts, ALT counts, ALT reverse counts or None)."""
    rng = np.random.default_rng(seed)
    sites = []
    z = lambda: np.zeros(S, np.int64)

    def one(s, v):
        a = z()
        a[s] = v
        return a

    def exact_depth(avg, nr_at):
        """avg * S reads in all, so avg_dp = avg exactly; the ALT reads as given ({sample: count})."""
        alt = z()
        for s, v in nr_at.items():
            alt[s] += v
        assert alt.sum() <= avg * S
        return _spread(avg * S - int(alt.sum()), S), alt, None

    sites.append((np.full(S, 5), z(), None))                                   # no ALT read
    if S > 1:
        sites.append((z(), one(0, 1), None))                                   # one read in all: avg_dp = 0
    sites.append(exact_depth(10, {0: 4}))                                      # nr / avg_dp = 0.4: M = 0 -> 1
    sites.append(exact_depth(10, {S - 1: 6, 0: 4} if S > 1 else {0: 10}))     # 1.0: M = 1 by rounding
    sites.append(exact_depth(10, {0: 10, S - 1: 5} if S > 1 else {0: 5}))     # 1.5 (one sample: 0.5): on the half, rounds up
    if S > 1:
        sites.append(exact_depth(10, {0: 10, 1: 7, S - 1: 3}))                 # 2.0: strictly inside 1..S (S >= 3)
        sites.append((_spread(4, S), _spread(10 * S - 4, S), None))            # S - 0.4: rounds to S
        sites.append((z(), _spread(2 * S - 1, S), None))                       # avg_dp = 1, nr = 2S - 1: clamped from above
        # M = 1 and q = 800: one sample has all the ALT reads, the others 540 REF reads each (nr / avg_dp = 1.48)
        sites.append((np.where(np.arange(S) == S // 2, 0, 540), one(S // 2, Q_LARGE), None))
        sites.append((np.full(S, 2), np.full(S, 3), None))                     # one bin takes every atomic
        sites.append((np.full(S, 1), rng.permutation(S) + 1, None))            # every count another
    # each of the chosen ALT depths at some sample
    for s0 in range(0, len(OI_VALUES), S):
        vals = OI_VALUES[s0:s0 + S]
        alt = z()
        alt[rng.choice(S, len(vals), replace=False)] = vals                    # (one sample, the value 0: a site without ALT)
        sites.append((np.full(S, 2), alt, None))
    # 511 and 512 at each of the chosen places, the other samples at 0..2
    for name, s in places(S).items():
        for v in (511, 512):
            alt = rng.integers(0, 3, S)
            alt[s] = v
            sites.append((rng.integers(1, 4, S), alt, None))
    # the deep cell
    alt = rng.integers(0, 3, S)
    rv = np.minimum(alt, 1)
    alt[DEEP_AT[S]], rv[DEEP_AT[S]] = DEEP_FWD + DEEP_REV, DEEP_REV
    sites.append((rng.integers(1, 4, S), alt, rv))
    return rng, sites


def sgb_tile(n_smpl, seed=None):
    rng, sites = site_counts(n_smpl, 940 + n_smpl if seed is None else seed)
    # a site without an ALT read between live ones (the indel form: a dead site), not at the tile's end
    sites.insert(len(sites) // 2, (np.full(n_smpl, 3), np.zeros(n_smpl, np.int64), None))
    return ss._tile_of_sites(n_smpl, [_site(rng, *s) for s in sites])


@functools.lru_cache(maxsize=None)
def sgb_case(n_smpl, indel=False):
    """(tile, cfg, the oracle's result): built once, shared, and left unchanged."""
    tile = sgb_tile(n_smpl)
    if indel:
        tile = ss.as_indel(tile)
    cfg = ss.make_cfg(tile)
    want = orc.mpileup(cfg, tile)
    for a in (tile.rd, tile.epos, tile.plp_off, tile.ref16) + ((tile.aux,) if indel else ()):
        a.setflags(write=False)
    return tile, cfg, want
