"""Directed inputs for the bias-test histograms and the site statistics (RPB, MQB, BQB, MQSB, VDB, FMT/SP), and a numpy
twin of one site's histograms.

The twin bins the accepted reads of a HostTile as bcf_call_glfgen does (bam2bcf.c:228-252) and takes the expected
statistics from the oracle's own routines on those arrays.  The generators below make every read accepted: base quality
at or above min_baseQ, neither RD_DEL nor RD_SKIP, a base other than N, epos in 0..99.

`wrapped16` is the model of what two 16-bit counters packed in one dword would hold.  A test uses it only to prove that
its input could detect a wrap: the value a statistic would take from wrapped histograms must differ from the true one.
"""
import ctypes as C
import functools
import math

import numpy as np

from bcftools_amd import abi, host
from . import orc

STATS = ("mwu_pos", "mwu_mq", "mwu_bq", "mwu_mqs", "vdb")
HISTS = ("ref_pos", "alt_pos", "ref_mq", "alt_mq", "ref_bq", "alt_bq", "fwd_mqs", "rev_mqs")
RTOL, ATOL = 2e-6, 1e-30           # assert_mplp_equal's comparison of the float site fields
FLAGS = abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD | abi.FMT_SP | abi.FMT_DP4
NT_A, NT_C = 1, 2                  # nt16 codes: the generators' reference base and their one ALT base
WG_CELLS = 256                     # cells of one glfgen workgroup


def make_cfg(tile):
    return abi.default_cfg(tile.n_smpl, max_sites=tile.n_sites, max_reads=len(tile.rd), fmt_flag=FLAGS)


# ---------------------------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------------------------
def read_fields(tile, lo, hi, min_baseQ=13, capQ=60):
    """The fields of reads [lo, hi) that the histograms are made of; asserts that every read is an accepted one."""
    w = tile.rd[lo:hi].astype(np.int64)
    assert not (w & (abi.RD_DEL | abi.RD_SKIP)).any()
    nt = (w >> 16) & 15
    if tile.is_indel:
        aux = tile.aux[lo:hi].astype(np.int64)
        bq = aux & 0xff
        diff = ((aux >> 16) & 0x3f) != 0
    else:
        bq = w & 0xff
        diff = None
        assert np.isin(nt, [1, 2, 4, 8]).all()
    assert (bq >= min_baseQ).all()
    mq = (w >> 8) & 0xff
    mq = np.minimum(np.where(mq == 255, 20, mq), capQ)
    ep = tile.epos[lo:hi].astype(np.int64)
    assert ep.max(initial=0) < 100
    return dict(bq=np.minimum(bq, 59), mq=np.minimum(mq, 59), nt=nt, rev=(w & abi.RD_REV) != 0, epos=ep, diff=diff)


def cell_range_hists(tile, site, c_lo, c_hi):
    """The eight histograms (int64) over the reads of cells [c_lo, c_hi) of `site`."""
    S = tile.n_smpl
    assert 0 <= c_lo <= c_hi <= S
    lo, hi = int(tile.plp_off[site * S + c_lo]), int(tile.plp_off[site * S + c_hi])
    f = read_fields(tile, lo, hi)
    # bam2bcf.c:247: REF when the read's nt16 code is the reference's; the indel pass has no reference base (-1)
    isref = np.zeros(hi - lo, bool) if tile.is_indel else f["nt"] == int(tile.ref16[site])
    h = {}
    for nm, key, n in (("pos", "epos", 100), ("mq", "mq", 60), ("bq", "bq", 60)):
        h["ref_" + nm] = np.bincount(f[key][isref], minlength=n).astype(np.int64)
        h["alt_" + nm] = np.bincount(f[key][~isref], minlength=n).astype(np.int64)
    h["fwd_mqs"] = np.bincount(f["mq"][~f["rev"]], minlength=60).astype(np.int64)
    h["rev_mqs"] = np.bincount(f["mq"][f["rev"]], minlength=60).astype(np.int64)
    return h


def site_hists(tile, site):
    return cell_range_hists(tile, site, 0, tile.n_smpl)


def wrapped16(lo, hi):
    """What the 16-bit halves of one dword hold after `lo` was added to the low and `hi` to the high half."""
    v = (np.asarray(lo, np.int64) + (np.asarray(hi, np.int64) << 16)) & 0xffffffff
    return v & 0xffff, v >> 16


def workgroup_pieces(tile, site, own=()):
    """The cell ranges of `site` that one workgroup's copy of the histograms takes: the site cut at multiples of 256 cells of
    the tile; a cell in `own` (a cell index of the tile: one worked on by a workgroup of its own) is a piece by itself."""
    S = tile.n_smpl
    cuts = {0, S}
    for c in range(site * S, (site + 1) * S + 1):
        if c % WG_CELLS == 0:
            cuts.add(c - site * S)
    for c in own:
        if site * S <= c < (site + 1) * S:
            cuts.update((c - site * S, c - site * S + 1))
    cuts = sorted(cuts)
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def wrapped_site_hists(tile, site, own=()):
    """The site's histograms if every workgroup kept its copy in packed 16-bit halves and added it up once, at its end."""
    tot = {k: np.zeros(100 if k.endswith("pos") else 60, np.int64) for k in HISTS}
    for a, b in workgroup_pieces(tile, site, own):
        h = cell_range_hists(tile, site, a, b)
        for lo, hi in (("ref_pos", "alt_pos"), ("ref_mq", "alt_mq"), ("ref_bq", "alt_bq"), ("fwd_mqs", "rev_mqs")):
            wl, wh = wrapped16(h[lo], h[hi])
            tot[lo] += wl
            tot[hi] += wh
    return tot


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def mwu(a, b):
    (a, pa), (b, pb) = _i32(a), _i32(b)
    assert len(a) == len(b)
    return orc.lib().orc_calc_mwu_bias(pa, pb, len(a))


def vdb(pos):
    pos, pp = _i32(pos)
    return orc.lib().orc_calc_vdb(pp, 100)


def stats_of(h):
    """The five statistics of a site from its histograms, as the float32 the site struct holds."""
    d = dict(mwu_pos=mwu(h["ref_pos"], h["alt_pos"]), mwu_mq=mwu(h["ref_mq"], h["alt_mq"]), mwu_bq=mwu(h["ref_bq"], h["alt_bq"]),
             mwu_mqs=mwu(h["fwd_mqs"], h["rev_mqs"]), vdb=vdb(h["alt_pos"]))
    with np.errstate(over="ignore"):
        return {k: np.float32(v) for k, v in d.items()}


def twin_stats(tile):
    """{statistic: float32[n_sites]} from the twin: STATS, and seg_bias from the cells' DP4 (sgb_twin)."""
    per = [stats_of(site_hists(tile, s)) for s in range(tile.n_sites)]
    out = {k: np.array([p[k] for p in per], np.float32) for k in STATS}
    out["seg_bias"] = twin_seg_bias(tile)
    return out


def cell_dp4(tile):
    """DP4 of every cell, int64 [n_sites][4][n_smpl]: REF forward, REF reverse, ALT forward, ALT reverse (anno[0..3])."""
    S, n = tile.n_smpl, tile.n_sites
    f = read_fields(tile, 0, len(tile.rd))
    cell = np.repeat(np.arange(n * S), np.diff(tile.plp_off.astype(np.int64)))
    if tile.is_indel:
        diff = f["diff"]
    else:
        ref = np.repeat(tile.ref16.astype(np.int64), np.add.reduceat(np.diff(tile.plp_off.astype(np.int64)), np.arange(0, n * S, S))) \
            if n else np.zeros(0, np.int64)
        assert np.isin(tile.ref16, [1, 2, 4, 8]).all()
        diff = f["nt"] != ref
    k = diff.astype(np.int64) * 2 + f["rev"]
    cnt = np.bincount(cell * 4 + k, minlength=n * S * 4).reshape(n, S, 4)
    return cnt.transpose(0, 2, 1)


def _log(x):
    return math.log(x) if x > 0 else -math.inf if x == 0 else math.nan


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def _logsumexp2(a, b):
    return _log(1 + _exp(b - a)) + a if a > b else _log(1 + _exp(a - b)) + b


def sgb_twin(anno, oi, n_smpl, clamp_hi=True, clamp_lo=True):
    """calc_SegBias (bam2bcf.c:494-530) in Python doubles, the per-sample terms added with math.fsum: (the value, the
    condition number sum |term| / |sum term|).  anno: the site's DP4 totals; oi: a sample's ALT reads, None for a sample
    that is left out of the sum (a model of a mistake; so are clamp_hi / clamp_lo = False, M without its clamps)."""
    nr = int(anno[2] + anno[3])
    if not nr:
        return math.inf, 0.0
    n = int(n_smpl)
    avg_dp = int((anno[0] + anno[1] + nr) / n)
    M = float(math.floor(nr / avg_dp + 0.5)) if avg_dp else math.inf
    if M > n:
        M = float(n) if clamp_hi else M
    elif M == 0 and clamp_lo:
        M = 1.0
    f = M / 2. / n
    p = nr / n
    q = nr / M if M else math.inf
    log2 = math.log(2.0)
    zero = _log(2 * f * (1 - f) * _exp(-q) + f * f * _exp(-2 * q) + (1 - f) * (1 - f)) + p
    terms = []
    for o in oi:
        if o is None:
            continue
        o = int(o)
        terms.append(_logsumexp2(_log(2 * (1 - f)), _log(f) + o * log2 - q) + (_log(f) + o * _log(q / p) - q + p) if o else zero)
    if not all(math.isfinite(t) for t in terms):
        return sum(terms), math.inf
    tot = math.fsum(terms)
    return tot, (math.fsum(abs(t) for t in terms) / abs(tot) if tot else math.inf)


def twin_seg_bias(tile):
    """seg_bias of every site as the float32 the site struct holds, from cell_dp4.  An indel site without a read of an indel
    type has no ALT allele: the record is dropped (bam2bcf.c:611) and every field of its site struct is 0."""
    d = cell_dp4(tile)
    out = np.zeros(tile.n_sites, np.float32)
    for s in range(tile.n_sites):
        anno = d[s].sum(axis=1)
        if tile.is_indel and not (anno[2] + anno[3]):
            continue
        with np.errstate(over="ignore"):
            out[s] = np.float32(sgb_twin(anno, d[s, 2] + d[s, 3], tile.n_smpl)[0])
    return out


def twin_sp(tile):
    d = cell_dp4(tile)
    out = np.zeros((tile.n_sites, tile.n_smpl), np.uint8)
    L = orc.lib()
    for s in range(tile.n_sites):
        for i in range(tile.n_smpl):
            a, b, c, e = (int(x) for x in d[s, :, i])
            if (a | b | c | e) > 0xffff:
                raise ValueError("DP4 past the 16-bit planes")
            out[s, i] = L.orc_format_sp(a, b, c, e)
    return out


def differs(x, y, factor=100.0):
    """x and y are further apart than `factor` times what the float comparison of the suite lets pass."""
    x, y = float(x), float(y)
    if math.isinf(x) or math.isinf(y):
        return math.isinf(x) != math.isinf(y)
    return abs(x - y) > factor * (RTOL * max(abs(x), abs(y)) + ATOL)


def mwu_int_products_ok(a, b):
    """calc_mwu_bias forms a[i] * nb as an int where b[i] == 0 (bam2bcf.c:455): below 2^31, else the reference is undefined."""
    nb = 0
    for x, y in zip(np.asarray(a, np.int64), np.asarray(b, np.int64)):
        if x and not y and int(x) * nb >= 1 << 31:
            return False
        nb += int(y)
    return True


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------
def _pack(bq, mq, nt, rev, tail=20):
    return (np.asarray(bq, np.int64) | np.asarray(mq, np.int64) << 8 | np.asarray(nt, np.int64) << 16
            | np.asarray(rev, np.int64) << 20 | np.int64(tail) << 24).astype(np.uint32)


def deep_site_tile(n_smpl, per_cell, seed, alt_frac, hot_ref, hot_alt, hot_epos=50, n_sites=1):
    """Cells of `per_cell` reads.  A read is ALT with probability alt_frac; it is "hot" with probability hot_ref (REF) or
    hot_alt (ALT).  A hot read has bq 40, mapQ 60 and epos = hot_epos (an int, or one value per site); the others have bq from
    {20, 30, 37, 40}, mapQ from {20, 40, 60} and epos uniform in 0..99.  Random strand, tail 20, reference A, ALT C."""
    rng = np.random.default_rng(seed)
    R = n_sites * n_smpl * per_cell
    alt = rng.random(R) < alt_frac
    hot = rng.random(R) < np.where(alt, hot_alt, hot_ref)
    he = np.repeat(np.broadcast_to(np.asarray(hot_epos, np.int64), (n_sites,)), n_smpl * per_cell)
    bq = np.where(hot, 40, rng.choice([20, 30, 37, 40], R))
    mq = np.where(hot, 60, rng.choice([20, 40, 60], R))
    ep = np.where(hot, he, rng.integers(0, 100, R))
    rd = _pack(bq, mq, np.where(alt, NT_C, NT_A), rng.integers(0, 2, R))
    off = np.arange(n_sites * n_smpl + 1, dtype=np.int64) * per_cell
    return host.HostTile(n_smpl, np.full(n_sites, NT_A, np.int8), off.astype(np.uint32), rd, ep.astype(np.uint8))


def as_indel(tile):
    """The same reads as a tile of the indel pass: aux = baseQ | seqQ << 8 | type << 16, type 0 for the REF reads and 1 for the
    others (the construction of tests/test_gpu_glfgen_fields.py's indel test)."""
    w = tile.rd.astype(np.int64)
    ref = np.repeat(tile.ref16.astype(np.int64), np.diff(tile.plp_off.astype(np.int64)[::tile.n_smpl]))
    ty = (((w >> 16) & 15) != ref).astype(np.int64)
    aux = ((w & 0xff) | 60 << 8 | ty << 16).astype(np.uint32)
    return host.HostTile(tile.n_smpl, np.zeros(tile.n_sites, np.int8), tile.plp_off, tile.rd, tile.epos, aux=aux, is_indel=1)


def exact_bins_tile():
    """Case A3.  64 cells of 1024 REF reads, 65 536 in all: every one at epos 50 and mapQ 40 on the forward strand (the REF bin
    of POS and of MQ and the forward bin of the strand histogram hold exactly 65 536), all but one at bq 40 (that REF bin
    holds exactly 65 535).  With exactly 65 536 reads in all there would be no ALT read and every statistic would be
    infinite whatever the counters did, so six cells carry one ALT read more: low qualities, three on either strand."""
    S, per = 64, 1024
    bq = np.full((S, per), 40, np.int64)
    bq[17, 500] = 30
    cells = []
    for i in range(S):
        rd = _pack(bq[i], 40, NT_A, 0)
        ep = np.full(per, 50, np.int64)
        if i < 6:
            rd = np.r_[rd[:300 + i], _pack([20 + 2 * i], [20], [NT_C], [i & 1]), rd[300 + i:]]
            ep = np.r_[ep[:300 + i], [5, 20, 35, 60, 80, 95][i], ep[300 + i:]]
        cells.append((rd, ep))
    off = np.r_[0, np.cumsum([len(c[0]) for c in cells])]
    return host.HostTile(S, np.array([NT_A], np.int8), off.astype(np.uint32), np.concatenate([c[0] for c in cells]),
                         np.concatenate([c[1] for c in cells]).astype(np.uint8))


LISTED_CELL = 5


def listed_cell_tile(seed=905):
    """37 samples, one site.  Cell 5 holds 40 000 forward and 40 000 reverse REF reads of bq 40, mapQ 60 and epos 50, and 3000
    ALT reads at spread positions: more entries than any key window, so it is listed and a workgroup of its own works on it.
    One ALT read in 25 has spread qualities too; were it every one, MQB and BQB would underflow to 0 whatever the counters
    did.  No base and strand of the cell has more than 65 535 reads.  The other cells are ordinary at depth 12."""
    rng = np.random.default_rng(seed)
    S = 37
    cells = []
    for i in range(S):
        if i == LISTED_CELL:
            n = 83000
            alt = np.zeros(n, bool)
            alt[rng.choice(n, 3000, replace=False)] = True
            rev = np.zeros(n, np.int64)
            rev[np.nonzero(~alt)[0][40000:]] = 1
            rev[alt] = rng.integers(0, 2, 3000)
            odd = alt & (rng.random(n) < 0.04)
            bq = np.where(odd, rng.choice([20, 30, 37, 40], n), 40)
            mq = np.where(odd, rng.choice([20, 40, 60], n), 60)
            ep = np.where(alt, rng.integers(0, 100, n), 50)
        else:
            n = 12
            alt = rng.random(n) < 0.3
            rev = rng.integers(0, 2, n)
            bq, mq, ep = rng.choice([20, 30, 37, 40], n), rng.choice([20, 40, 60], n), rng.integers(0, 100, n)
        cells.append((_pack(bq, mq, np.where(alt, NT_C, NT_A), rev), ep))
    off = np.r_[0, np.cumsum([len(c[0]) for c in cells])]
    return host.HostTile(S, np.array([NT_A], np.int8), off.astype(np.uint32), np.concatenate([c[0] for c in cells]),
                         np.concatenate([c[1] for c in cells]).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# part A's cases: name -> (builder, group, the statistics the case claims, cells with a workgroup of their own)
# A case claims a statistic when, at some site, its true value is further than 100 x the comparison tolerance from the value
# wrapped counters would give.  tests/test_oracle_site_stats.py asserts every claim.
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, build, group, claims, own=()):
        self.build, self.group, self.claims, self.own = build, group, tuple(claims), tuple(own)


A1 = dict(n_smpl=64, per_cell=1100, seed=901, alt_frac=0.03, hot_ref=0.985, hot_alt=0.93, hot_epos=50)
A2 = dict(n_smpl=64, per_cell=2600, seed=902, alt_frac=0.5, hot_ref=0.985, hot_alt=0.90, hot_epos=50)
SLOT_EPOS = [50, 23, 50, 71, 50, 8, 50, 96]      # every second site another hot epos

DEEP_CASES = {
    # one workgroup, one slot
    "A1": Case(lambda: deep_site_tile(**A1), "one_wg", ["mwu_pos", "mwu_mq", "mwu_bq"]),
    "A2": Case(lambda: deep_site_tile(**A2), "one_wg", ["mwu_pos", "mwu_mqs"]),
    "A3": Case(exact_bins_tile, "one_wg", ["mwu_pos", "mwu_mq", "mwu_mqs", "vdb"]),
    # two workgroups on one site: 256 + 44 cells
    "two_wg_half": Case(lambda: deep_site_tile(300, 560, 903, 0.5, 0.985, 0.90), "two_wg", ["mwu_pos", "mwu_mqs"]),
    "two_wg_alt3": Case(lambda: deep_site_tile(300, 560, 904, 0.03, 0.985, 0.93), "two_wg", ["mwu_mq", "mwu_bq"]),
    # (a handful of ALT reads: the carry out of the REF half is a read more at the hot epos, which VDB of a few reads shows)
    "two_wg_few_alt": Case(lambda: deep_site_tile(300, 560, 906, 6e-5, 0.985, 0.0), "two_wg", ["mwu_pos", "vdb"]),
    # several slots: 37 samples, the smallest LDS form, eight slots
    "slots": Case(lambda: deep_site_tile(37, 1800, 907, 0.002, 0.995, 0.90, hot_epos=SLOT_EPOS, n_sites=8), "slots",
                  ["mwu_pos", "mwu_mq", "mwu_bq"]),
    # the global form (32-bit counters): nothing packed, nothing claimed
    "control": Case(lambda: deep_site_tile(36, 1900, 908, 0.002, 0.995, 0.90, hot_epos=[50, 23], n_sites=2), "control", []),
    "listed": Case(listed_cell_tile, "listed", ["mwu_pos", "mwu_mq", "mwu_bq", "vdb"], own=[LISTED_CELL]),
    # the indel instantiation (no reference base: every read is in the ALT arrays, RPB, MQB and BQB are infinite)
    # A1 as an indel tile cannot show a wrap (VDB underflows to 0 with or without it): a parity run at depth, nothing more
    "A1_indel": Case(lambda: as_indel(deep_site_tile(**A1)), "indel", []),
    "A2_indel": Case(lambda: as_indel(deep_site_tile(**A2)), "indel", ["mwu_mqs"]),
    # 42 % of the reads at one epos (70 000 in the ALT half of that bin), the others spread: VDB stays well above 0 and moves
    # when the half loses its top
    "spread_indel": Case(lambda: as_indel(deep_site_tile(64, 2600, 909, 0.5, 0.42, 0.42)), "indel", ["vdb"]),
}


@functools.lru_cache(maxsize=None)
def deep_case(name):
    """(tile, cfg, the oracle's result) of a case of part A: built once, shared, and left unchanged."""
    tile = DEEP_CASES[name].build()
    cfg = make_cfg(tile)
    want = orc.mpileup(cfg, tile)
    for a in (tile.rd, tile.epos, tile.plp_off, tile.ref16):
        a.setflags(write=False)
    return tile, cfg, want


# ---------------------------------------------------------------------------------------------------------------------
# part B: the regimes of the statistics
# ---------------------------------------------------------------------------------------------------------------------
GRID = (0, 1, 2, 3, 5, 7, 8, 9, 20)
VDB_DEPTHS = (4, 10, 12, 15, 100, 150, 199, 200, 201)
VDB_ROWS = (3, 4, 5, 6, 7, 8, 9, 10, 15, 20, 30, 40, 50, 100, 200)           # calc_vdb's table rows (bam2bcf.c:287-291)
LEVELS = dict(bq=(20, 30, 40), mq=(20, 40, 60), epos=(10, 50, 90))
SEPARATED = ((3, 3), (5, 7), (7, 5), (7, 7), (2, 5), (8, 3), (20, 20))
# DP4 tables (REF forward, REF reverse, ALT forward, ALT reverse) of chosen cells
SP_TABLES = (
    (0, 0, 5, 5), (5, 5, 0, 0), (0, 5, 0, 5), (5, 0, 5, 0),                   # each margin at 0
    (1, 0, 5, 5), (5, 5, 0, 1), (1, 5, 0, 5), (5, 0, 5, 1),                   # ... and at 1
    (2, 0, 0, 2), (1, 1, 1, 1),                                               # every margin at 2: the smallest tables that are tested
    (20, 20, 20, 20), (22, 18, 18, 22), (33, 7, 7, 33), (11, 29, 29, 11),     # walks over n11 = 11, 22 and 33
    (1500, 1500, 1500, 1500), (1600, 1400, 1400, 1600),                       # cells past 255 reads: balanced,
    (2000, 1000, 1000, 2000), (900, 600, 500, 1000),                          # one-sided (p above the smallest double:
                                                                              # below it the reference takes log(0)),
    (60, 0, 0, 60),                                                           # and a Phred value past 255
)


def _tile_of_sites(n_smpl, sites):
    """sites: a list of dicts of equal-length per-read arrays smpl, bq, mq, alt, rev, epos and, if not 20 throughout, tail."""
    rd, ep, cnt = [], [], []
    for s in sites:
        o = np.argsort(s["smpl"], kind="stable")
        rd.append(_pack(s["bq"][o], s["mq"][o], np.where(s["alt"][o], NT_C, NT_A), s["rev"][o], s["tail"][o] if "tail" in s else 20))
        ep.append(s["epos"][o])
        cnt.append(np.bincount(s["smpl"], minlength=n_smpl))
    off = np.r_[0, np.cumsum(np.concatenate(cnt))]
    return host.HostTile(n_smpl, np.full(len(sites), NT_A, np.int8), off.astype(np.uint32), np.concatenate(rd),
                         np.concatenate(ep).astype(np.uint8))


def regime_tile(n_smpl, seed):
    """One tile whose sites walk the regimes of calc_mwu_bias, calc_vdb and FMT/SP; a site's reads are dealt over the samples.
      grid   (n_ref, n_alt) in GRID x GRID, strands dealt so that (n_fwd, n_rev) is in GRID x GRID too where the total
             allows; base quality, mapQ and epos each from three levels (ties: half-integer U)
      sep    REF and ALT completely separated in all three values, either way, REF forward and ALT reverse (so the strand
             test sees the same): U = 0 and U = na * nb, with na = nb = 7 among them
      vdb    ALT depths on, between and past the rows of calc_vdb's table, all at epos 0, all at 99, uniform
      sp     cells with chosen DP4 tables (SP_TABLES)"""
    rng = np.random.default_rng(seed)
    sites = []

    def site(n, alt, rev, bq=None, mq=None, epos=None, smpl=None):
        lv = lambda k: rng.choice(LEVELS[k], n)
        return dict(smpl=rng.integers(0, n_smpl, n) if smpl is None else smpl, alt=np.asarray(alt, bool), rev=np.asarray(rev, np.int64),
                    bq=lv("bq") if bq is None else bq, mq=lv("mq") if mq is None else mq, epos=lv("epos") if epos is None else epos)

    for k, (nr, na) in enumerate((a, b) for a in GRID for b in GRID):
        T = nr + na
        fit = [f for f in GRID if T - f in GRID]
        nf = fit[k % len(fit)] if fit else T // 2
        sites.append(site(T, np.arange(T) >= nr, rng.permutation(np.arange(T) >= nf)))
    for nr, na in SEPARATED:
        for up in (0, 1):                                    # REF below ALT, REF above ALT
            alt = np.arange(nr + na) >= nr
            hi = alt == bool(up)
            pick = lambda k: np.where(hi, LEVELS[k][2], LEVELS[k][0])
            # (mapQ levels 20 and 40: both below the mapQ >= 59 bin's separate path, which the grid sites take)
            sites.append(site(nr + na, alt, alt, bq=pick("bq"), mq=np.where(hi, 40, 20), epos=pick("epos")))
    for d in VDB_DEPTHS:
        for how in (0, 99, None):
            n = d + 3
            alt = np.arange(n) >= 3
            ep = rng.integers(0, 100, n) if how is None else np.where(alt, how, rng.integers(0, 100, n))
            sites.append(site(n, alt, rng.integers(0, 2, n), epos=ep))
    for s0 in range(0, len(SP_TABLES), n_smpl):
        parts = []
        for i, t in enumerate(SP_TABLES[s0:s0 + n_smpl]):
            for j, c in enumerate(t):
                parts.append((np.full(c, i), np.full(c, j >= 2), np.full(c, j & 1)))
        smpl, alt, rev = (np.concatenate([p[x] for p in parts]) for x in range(3))
        sites.append(site(len(smpl), alt, rev, epos=rng.integers(0, 100, len(smpl)), smpl=smpl))
    return _tile_of_sites(n_smpl, sites)


def replay_tile(seed=911):
    """64 samples x 5400 ALT reads at uniform positions (and one REF read a cell): the sum of pos * i is past 2^24, where
    calc_vdb's float sum stops being the integer total.  Qualities spread over many bins: none is near 2^16."""
    rng = np.random.default_rng(seed)
    S, per = 64, 5401
    R = S * per
    alt = np.tile(np.arange(per) != 2000, S)
    rd = _pack(rng.integers(13, 60, R), rng.integers(1, 59, R), np.where(alt, NT_C, NT_A), rng.integers(0, 2, R))
    return host.HostTile(S, np.array([NT_A], np.int8), (np.arange(S + 1) * per).astype(np.uint32), rd, rng.integers(0, 100, R).astype(np.uint8))


def _mwu_sums(a, b):
    na = nb = 0
    U = 0.0
    for x, y in zip((int(v) for v in a), (int(v) for v in b)):
        if x:
            U += x * (nb + y * 0.5)
            na += x
        nb += y
    return na, nb, U


def mwu_regimes(a, b):
    na, nb, U = _mwu_sums(a, b)
    if not na or not nb:
        return {"zero"}
    if na == 1 or nb == 1:
        return {"one"}
    if na == 2 or nb == 2:
        return {"two"}
    if na >= 8 or nb >= 8:
        return {"normal"}
    out = {"exact", "exact_half" if U != int(U) else "exact_whole"}
    if U == 0:
        out.add("exact_U0")
    if U == na * nb:
        out.add("exact_Umax")
    if na == 7 and nb == 7 and U in (0, 49):
        out.add("exact_7_7_U%d" % int(U))
    return out


def vdb_regimes(pos):
    dp = int(np.sum(pos))
    if dp < 2:
        return {"lt2"}
    if dp == 2:
        return {"eq2"}
    pos = np.asarray(pos, np.int64)
    out = {"ge200" if dp >= 200 else "row" if dp in VDB_ROWS else "between"}
    # where the reads are: all at epos 0, all at 99, or over several bins
    how = "all0" if pos[0] == dp else "all99" if pos[99] == dp else "spread" if np.count_nonzero(pos) > 1 else None
    if how:
        out |= {how, next(iter(out)) + "_" + how}
    if int(np.dot(np.asarray(pos, np.int64), np.arange(len(pos)))) >= 1 << 24:
        out.add("replay")
    return out


def fisher_walk(a, b, c, d):
    """The n11 at which kt_fisher_exact (htslib kfunc.c) asks hypergeo_acc for the next term of a tail: up from the smallest
    and down from the largest n11 the margins allow, each until a term reaches the table's own probability."""
    n1_, n_1, n = a + b, a + c, a + b + c + d
    lo, hi = max(0, n1_ + n_1 - n), min(n1_, n_1)
    if lo == hi:
        return set()
    lb = lambda N, k: math.lgamma(N + 1) - math.lgamma(k + 1) - math.lgamma(N - k + 1)
    pmf = lambda k: math.exp(lb(n1_, k) + lb(n - n1_, n_1 - k) - lb(n, n_1))
    q, seen = pmf(a), set()
    p, i = pmf(lo), lo + 1
    while p < 0.99999999 * q and i <= hi:
        seen.add(i)
        p, i = pmf(i), i + 1
    p, j = pmf(hi), hi - 1
    while p < 0.99999999 * q and j >= 0:
        seen.add(j)
        p, j = pmf(j), j - 1
    return seen


def sp_regimes(t):
    a, b, c, d = (int(x) for x in t)
    m = (a + b, c + d, a + c, b + d)
    out = set()
    for k in range(4):
        if m[k] < 2:
            out.add("margin%d_at_%d" % (k, m[k]))
    if out:
        return out
    n1_, n_1, n = a + b, a + c, a + b + c + d
    lo, hi = max(0, n1_ + n_1 - n), min(n1_, n_1)
    sp = orc.lib().orc_format_sp(a, b, c, d)
    # hypergeo_acc forms a term afresh, not from its neighbour, where n11 is a multiple of 11 (kfunc.c)
    out |= {"anchor%d" % k for k in (11, 22, 33) if k in fisher_walk(a, b, c, d)}
    if max(a, b, c, d) > 255:
        out.add("deep_one_sided" if sp >= 100 else "deep_balanced")
    if sp == 255:
        out.add("cap255")
    return out or {"plain"}


MWU_NEED = {"zero", "one", "two", "exact", "exact_half", "exact_U0", "exact_Umax", "exact_7_7_U0", "exact_7_7_U49", "normal"}
VDB_NEED = {"lt2", "eq2"} | {r + h for r in ("row", "between", "ge200") for h in ("", "_all0", "_all99", "_spread")}
SP_NEED = {"margin%d_at_%d" % (k, v) for k in range(4) for v in (0, 1)} | {"anchor11", "anchor22", "anchor33", "deep_one_sided", "deep_balanced", "cap255", "plain"}


def regimes(tile):
    """{statistic: the regimes that occur in the tile}, from the twin's counts."""
    seen = {k: set() for k in STATS + ("sp",)}
    for s in range(tile.n_sites):
        h = site_hists(tile, s)
        seen["mwu_pos"] |= mwu_regimes(h["ref_pos"], h["alt_pos"])
        seen["mwu_mq"] |= mwu_regimes(h["ref_mq"], h["alt_mq"])
        seen["mwu_bq"] |= mwu_regimes(h["ref_bq"], h["alt_bq"])
        seen["mwu_mqs"] |= mwu_regimes(h["fwd_mqs"], h["rev_mqs"])
        seen["vdb"] |= vdb_regimes(h["alt_pos"])
    d = cell_dp4(tile)
    for t in {tuple(x) for x in d.transpose(0, 2, 1).reshape(-1, 4).tolist()}:
        seen["sp"] |= sp_regimes(t)
    return seen


def assert_regime_coverage(tile):
    seen = regimes(tile)
    for k in ("mwu_pos", "mwu_mq", "mwu_bq", "mwu_mqs"):
        assert MWU_NEED <= seen[k], (k, sorted(MWU_NEED - seen[k]))
    assert VDB_NEED <= seen["vdb"], sorted(VDB_NEED - seen["vdb"])
    assert SP_NEED <= seen["sp"], sorted(SP_NEED - seen["sp"])


@functools.lru_cache(maxsize=None)
def regime_case(n_smpl):
    """(tile, cfg, the oracle's result); n_smpl 0: the replay tile."""
    tile = regime_tile(n_smpl, 920 + n_smpl) if n_smpl else replay_tile()
    cfg = make_cfg(tile)
    want = orc.mpileup(cfg, tile)
    for a in (tile.rd, tile.epos, tile.plp_off, tile.ref16):
        a.setflags(write=False)
    return tile, cfg, want
