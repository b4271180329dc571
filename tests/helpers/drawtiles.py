"""The tiles of the draw tests (tests/test_oracle_draw_twin.py on the CPU, tests/test_gpu_draw_forms.py on the device), built
once and shared, with what the twin (tests/helpers/drawtwin.py) and the oracle say about each.

One read generator serves every tile: base qualities on both sides of every min_baseQ in use, mapQ 0 and 255, every nt16 code,
both strands, the soft-clip bit, deletions and ref-skips, reference code 15.  A cell is given as (usable reads, other entries),
so that a tile can hold exactly the cells a test is about; the entries of a cell are in random order.

The bases of a site are unevenly spread over its four alleles, each cell with fractions of its own: the site's allele order
(bcf_call_combine's qsum ranking, over all reads) is then the same with and without the reads a deep cell drops, so the PLs of
the twin-reduced tile line up with the whole tile's, while cells between a homozygous and a heterozygous call keep PLs below the
255 cap that change with the reads taken."""
import functools

import numpy as np

from bcftools_amd import abi, host
from tests.helpers import drawtwin, orc

GLF_MAX_WINDOW = 16384            # csrc/kernels.h: the most keys a workgroup's LDS window ever holds
QUALS = np.array([2, 12, 13, 14, 25, 29, 30, 31, 37, 40])
MAPQ = np.array([0, 20, 60, 60, 60, 255])
OTHER_NT16 = np.array([0, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15])
P_DEL, P_SKIP = 0.03, 0.02
FMT = abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD | abi.FMT_QS | abi.FMT_SCR | abi.INFO_SCR | abi.FMT_SP
PLANES = ("pl", "dp4", "adf", "adr", "qs", "scr")
EXACT_SITE = ("anno", "depth", "ori_depth", "mq0")


def _p_low(min_baseQ):
    return float((QUALS < min_baseQ).mean())


def ordinary(rng, n_cells, mean, min_baseQ, is_indel=False):
    """(usable, other) entries of ordinary cells: Poisson depth, each read a deletion, a ref-skip or a base of any quality."""
    e = rng.poisson(mean, n_cells)
    p_not = P_SKIP if is_indel else 1.0 - (1.0 - P_DEL - P_SKIP) * (1.0 - _p_low(min_baseQ))
    n_not = rng.binomial(e, p_not)
    return (e - n_not).astype(np.int64), n_not.astype(np.int64)


def make_tile(rng, n_sites, n_smpl, n_use, n_not, min_baseQ, is_indel=False):
    n_use, n_not = np.asarray(n_use, np.int64), np.asarray(n_not, np.int64)
    n_cells = n_sites * n_smpl
    assert len(n_use) == len(n_not) == n_cells
    dep = n_use + n_not
    off = np.r_[0, np.cumsum(dep)]
    R = int(off[-1])
    cell = np.repeat(np.arange(n_cells), dep)
    site = cell // n_smpl
    within = np.lexsort((rng.random(R), cell))                  # a random order inside every cell
    use = np.empty(R, bool)
    use[within] = (np.arange(R) - off[cell]) < n_use[cell]
    qual = rng.choice(QUALS, R)
    flag = np.zeros(R, np.int64)
    if is_indel:
        flag[use & (rng.random(R) < P_DEL)] |= abi.RD_DEL      # a deletion at the site is a read of the indel pass
        flag[~use] |= abi.RD_SKIP
        flag[~use & (rng.random(R) < 0.2)] |= abi.RD_DEL
    else:
        ok = QUALS[QUALS >= min_baseQ]
        qual[use] = rng.choice(ok, int(use.sum()))
        w = np.array([P_DEL, P_SKIP, (1.0 - P_DEL - P_SKIP) * _p_low(min_baseQ)])
        kind = rng.choice(3, R, p=w / w.sum())
        flag[~use & (kind == 0)] |= abi.RD_DEL
        flag[~use & (kind == 1)] |= abi.RD_SKIP
        flag[~use & (kind == 1) & (rng.random(R) < 0.2)] |= abi.RD_DEL
        low = ~use & (kind == 2)
        if low.any():
            qual[low] = rng.choice(QUALS[QUALS < min_baseQ], int(low.sum()))
    # the bases: the site's alleles in an order of its own, each cell with its own share of the second to fourth
    f = np.stack([np.full(n_cells, 0.04), rng.uniform(0.003, 0.015, n_cells), rng.uniform(0.02, 0.07, n_cells), rng.uniform(0.02, 0.25, n_cells)], 1)
    rank = (rng.random(R)[:, None] >= np.cumsum(f, 1)[cell]).sum(1)               # 0: another code, 1..3: fourth..second allele, 4: the first
    alleles = np.stack([rng.permutation([1, 2, 4, 8]) for _ in range(n_sites)])
    nt16 = np.where(rank == 0, rng.choice(OTHER_NT16, R), alleles[site, np.maximum(4 - rank, 0) % 4])
    rd = (qual | (rng.choice(MAPQ, R) << 8) | (nt16 << 16) | (rng.integers(0, 2, R) << 20) | ((rng.random(R) < 0.1).astype(np.int64) << 21)
          | flag | (rng.integers(0, 40, R) << 24)).astype(np.uint32)
    aux = None
    if is_indel:
        g = np.stack([rng.uniform(0, 0.02, n_cells), rng.uniform(0, 0.03, n_cells), rng.uniform(0, 0.08, n_cells), rng.uniform(0.02, 0.3, n_cells)], 1)
        typ = np.maximum(4 - (rng.random(R)[:, None] >= np.cumsum(g, 1)[cell]).sum(1), 0)   # 4, 3, 2, 1 with the cell's shares, else 0
        aux = ((typ << 16) | (rng.integers(20, 60, R) << 8) | rng.choice(QUALS, R)).astype(np.uint32)
    ref16 = rng.choice([1, 2, 4, 8, 15], n_sites).astype(np.int8)
    return host.HostTile(n_smpl, ref16, off.astype(np.uint32), rd, rng.integers(0, 100, R).astype(np.uint8), aux=aux, is_indel=1 if is_indel else 0)


def cell_counts(tile, min_baseQ):
    """(entries, usable reads) of every cell, counted from the tile as it stands."""
    off = tile.plp_off.astype(np.int64)
    c = np.r_[0, np.cumsum(drawtwin.usable(tile, min_baseQ))]
    return np.diff(off), c[off[1:]] - c[off[:-1]]


class Case:
    def __init__(self, snp, min_baseQ=13, indel=None, cols=None, ret=None, visit=None, listed=()):
        self.snp, self.indel, self.min_baseQ = snp, indel, min_baseQ
        self.cols = None if cols is None else np.asarray(cols, np.int32)
        self.ret = None if ret is None else np.asarray(ret, np.int32)
        self.visit = None if visit is None else np.asarray(visit, np.uint8)
        self.n_smpl = snp.n_smpl
        self.entries, self.n_use = cell_counts(snp, min_baseQ)
        self.deep = self.n_use > abi.MAX_DEPTH
        self.listed = np.asarray(listed, np.int64)               # cells meant for the DEEP = true launch
        self.max_reads = max(len(snp.rd), 0 if indel is None else len(indel.rd))

    def cfg(self, max_reads=None, max_sites=None):
        return abi.default_cfg(self.n_smpl, max_sites=max_sites or self.snp.n_sites, max_reads=max_reads or self.max_reads, fmt_flag=FMT,
                               min_baseQ=self.min_baseQ)

    @property
    def hist_slots(self):
        """csrc/api.hip: the LDS-histogram form of glfgen_kernel is taken when a workgroup's 256 cells span at most 8 sites."""
        return 255 // self.n_smpl + 2


def _deep_tile(seed, n_smpl, n_sites, min_baseQ, fixed, n_deep, lo=256, hi=700, is_indel=False):
    """Ordinary cells of about 12 reads; `fixed`: {cell: (usable, other)}; further deep cells of lo..hi usable reads at random
    places until there are n_deep."""
    rng = np.random.default_rng(seed)
    n_cells = n_smpl * n_sites
    nu, nn = ordinary(rng, n_cells, 12, min_baseQ, is_indel)
    for c, (u, o) in fixed.items():
        nu[c], nn[c] = u, o
    have = sum(1 for u, _ in fixed.values() if u > abi.MAX_DEPTH)
    free = np.setdiff1d(np.arange(n_cells), list(fixed))
    for c in rng.choice(free, max(n_deep - have, 0), replace=False):
        nu[c], nn[c] = rng.integers(lo, hi + 1), rng.integers(0, 40)
    return make_tile(rng, n_sites, n_smpl, nu, nn, min_baseQ, is_indel)


@functools.lru_cache(maxsize=None)
def lds(min_baseQ=13, seed=101):
    """48 samples x 6 sites: the LDS-histogram form, 288 cells (two workgroups of draw_scan_kernel), more than 64 deep cells (two
    workgroups of draw_shuffle_kernel); the first and the last cell deep, two deep neighbours, cells of exactly 255, 256 and 257
    usable reads among more entries, one cell of many entries and few usable reads."""
    S, n_sites = 48, 6
    fixed = {0: (411, 9), S * n_sites - 1: (305, 4), 100: (520, 12), 101: (333, 0), 30: (255, 10), 31: (256, 10), 200: (257, 10), 260: (200, 120)}
    c = Case(_deep_tile(seed, S, n_sites, min_baseQ, fixed, 72), min_baseQ)
    c.snp.ref16[3] = 15
    assert c.deep[0] and c.deep[-1] and c.deep[100] and c.deep[101] and 100 // S == 101 // S
    for cell, u in ((30, 255), (31, 256), (200, 257)):
        assert c.n_use[cell] == u and c.entries[cell] > 257
    assert c.entries[260] > abi.MAX_DEPTH >= c.n_use[260]
    return c


@functools.lru_cache(maxsize=None)
def lds_other(seed=202):
    """A second, different tile of the same form (the generator across calls)."""
    return Case(_deep_tile(seed, 48, 5, 13, {7: (256, 3), 150: (640, 20)}, 40), 13)


@functools.lru_cache(maxsize=None)
def glob(seed=303):
    """3 samples x 30 sites: the global-histogram form at the same density of deep cells."""
    return Case(_deep_tile(seed, 3, 30, 13, {0: (300, 5), 89: (277, 0)}, 72), 13)


@functools.lru_cache(maxsize=None)
def listed(n_smpl, n_sites, seed):
    """Two cells of more than GLF_MAX_WINDOW entries (listed whatever window the tile's mean depth selects): one with 300..600
    usable reads, one with at most 255, which spends no draw; one ordinary deep cell of 300 usable reads."""
    n_cells = n_smpl * n_sites
    a, b, d = (17, 250, 100) if n_sites == 1 else (5, n_cells - 1, 60)
    fixed = {a: (300 + 37 * n_sites, GLF_MAX_WINDOW + 116), b: (200, GLF_MAX_WINDOW + 16), d: (300, 6)}
    c = Case(_deep_tile(seed, n_smpl, n_sites, 13, fixed, 2), 13, listed=(a, b))
    assert (c.entries[[a, b]] > GLF_MAX_WINDOW).all() and 300 <= c.n_use[a] <= 600 and c.n_use[b] <= abi.MAX_DEPTH
    assert c.n_use[d] == 300 and c.entries[d] <= 2048 and c.deep.sum() == 2
    return c


@functools.lru_cache(maxsize=None)
def filled(n_smpl, n_sites, seed):
    """Every cell exactly 256 entries, all usable: n_reads / 256 deep cells, one below the bound of the lists."""
    n = n_smpl * n_sites
    c = Case(make_tile(np.random.default_rng(seed), n_sites, n_smpl, np.full(n, 256), np.zeros(n, np.int64), 13), 13)
    assert (c.entries == 256).all() and (c.n_use == 256).all() and len(c.snp.rd) == 256 * n
    return c


@functools.lru_cache(maxsize=None)
def both(seed=404):
    """48 samples, 6 SNP columns, indel sites at columns 1, 3 and 4, the one at column 3 with a gap_prep return of -1; column 2
    lies outside the targets.  Deep cells in both passes, also where the pass does not run."""
    S = 48
    snp = _deep_tile(seed, S, 6, 13, {2 * S + 5: (400, 7), 3: (256, 2), 6 * S - 1: (290, 0)}, 14)
    indel = _deep_tile(seed + 1, S, 3, 13, {1 * S + 9: (350, 5), 0: (257, 3), 3 * S - 1: (480, 11)}, 9, is_indel=True)
    c = Case(snp, 13, indel=indel, cols=[1, 3, 4], ret=[0, -1, 0], visit=[1, 1, 0, 1, 1, 1])
    c.i_entries, c.i_use = cell_counts(indel, 13)
    c.i_deep = c.i_use > abi.MAX_DEPTH
    return c


@functools.lru_cache(maxsize=None)
def cohort(seed=505):
    """300 samples x 3 sites with deep cells that fit the window (the fused pipeline's many-sample launch set)."""
    return Case(_deep_tile(seed, 300, 3, 13, {0: (256, 1), 899: (300, 0)}, 20), 13)


def rows(res, idx):
    """The sites `idx` of an MplpResult as a result of their own."""
    out = host.MplpResult(len(idx), res.n_smpl)
    for k in ("site", "pl", "dp4", "adf", "adr", "qs", "scr", "sp"):
        getattr(out, k)[:] = getattr(res, k)[idx]
    return out


class Refs:
    """What the twin and the oracle say about a case: keep masks, generator states, and the oracle's planes under the draw
    (`want`), under the first-255 rule (`first`) and, first-255 again, on the twin-reduced tile (`red`); `*_i`: the indel pass."""


def _snp_refs(c, reset, start):
    r = Refs()
    (r.keep, _), r.twin_state, r.n_deep = drawtwin.draw(c.snp, min_baseQ=c.min_baseQ, state=start)
    r.reduced = drawtwin.reduced(c.snp, r.keep)
    cfg = c.cfg()
    r.want = orc.mpileup(cfg, c.snp, deep_rule=0, reset=reset)
    r.orc_state = int(orc.lib().orc_rand48_state())
    r.first = orc.mpileup(cfg, c.snp, deep_rule=1)
    r.red = orc.mpileup(cfg, r.reduced, deep_rule=1)
    return r


@functools.lru_cache(maxsize=None)
def refs(case):
    """case: a Case of a SNP-only tile, drawn from a fresh generator."""
    return _snp_refs(case, True, drawtwin.SEED)


@functools.lru_cache(maxsize=None)
def refs_chain(first, second):
    """Two tiles one after the other on one generator: (Refs of the first, Refs of the second)."""
    a = refs(first)
    orc.mpileup(first.cfg(), first.snp, deep_rule=0, reset=True)             # puts the oracle's generator where the first tile leaves it
    assert int(orc.lib().orc_rand48_state()) == a.orc_state
    return a, _snp_refs(second, False, a.twin_state)


@functools.lru_cache(maxsize=None)
def refs_both(c):
    """The two-pass case: the oracle site by site in mpileup_reg()'s order over the visited columns."""
    from tests.test_gpu_draw import _oracle_in_visit_order
    r = Refs()
    (r.keep, r.keep_i), r.twin_state, r.n_deep = drawtwin.draw(c.snp, c.indel, c.cols, c.ret, c.visit, c.min_baseQ)
    r.reduced, r.reduced_i = drawtwin.reduced(c.snp, r.keep), drawtwin.reduced(c.indel, r.keep_i)
    cfg = c.cfg()
    r.kept = np.nonzero(c.visit)[0]
    r.live = c.ret == 0
    col_in_kept = [int(np.nonzero(r.kept == col)[0][0]) for col in c.cols]           # every indel site lies at a visited column
    r.want, r.want_i, r.orc_state = _oracle_in_visit_order(cfg, c.snp.select_sites(r.kept), c.indel, col_in_kept, c.ret)
    r.first, r.first_i = orc.mpileup(cfg, c.snp, deep_rule=1), orc.mpileup(cfg, c.indel, deep_rule=1)
    r.red, r.red_i = orc.mpileup(cfg, r.reduced, deep_rule=1), orc.mpileup(cfg, r.reduced_i, deep_rule=1)
    return r


def deep_cells_differ(a, b, deep):
    """In how many of the cells `deep` two results' PLs differ."""
    d = (a.pl != b.pl).any(axis=1).reshape(-1)                   # [site][sample] -> cell
    return int((d & deep).sum())
