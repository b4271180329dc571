"""glfgen_kernel's straight-line code around its loops, on the cells that reach it rarely:

  A  a cell with reads of two or more bases gets its 15 likelihoods from 15 lanes of its wavefront, one cell after the other;
  B  a wavefront in which no cell has two reads off the primary base forms each such read's sum as one product.

Crafted cells among ordinary ones, compared field by field and bit for bit with the oracle, in a tile of 64 samples (histograms
in LDS) and in one of 4 (global histograms); tiles of 300 to 600 cells: two workgroups, the last one ragged.  PL stops at 255,
so every crafted cell of two or more bases first shows, on the oracle's likelihoods, that it is not saturated: a wrong sum is
then a wrong PL."""
import os
import re

import numpy as np
import pytest

from bcftools_amd import abi, host
from tests.helpers import orc
from tests.test_gpu_parity import assert_mplp_equal, EXACT_SITE, FLOAT_SITE

gpu = pytest.mark.gpu

FMT = abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD | abi.FMT_QS | abi.FMT_SP
SAMPLES = [64, 4]                 # hist_slots > 0 (n_smpl >= 37) and the global-histogram form
GLFGEN_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bcftools_amd", "csrc", "glfgen.hip")


def test_genotype_table_is_tri_order():
    """The (j, k) a lane forms its likelihood for, a nibble a lane in GLF_TRI_J / GLF_TRI_K: lane z holds the z-th pair of
    tri(j, k) = k (k + 1) / 2 + j over j <= k < 5, and the lanes past the 15 likelihoods hold (0, 0)."""
    src = open(GLFGEN_HIP).read()
    tj = int(re.search(r"#define\s+GLF_TRI_J\s+0x([0-9a-fA-F]+)ull", src).group(1), 16)
    tk = int(re.search(r"#define\s+GLF_TRI_K\s+0x([0-9a-fA-F]+)ull", src).group(1), 16)
    pairs = sorted(((k * (k + 1) // 2 + j, j, k) for k in range(5) for j in range(k + 1)))
    assert [z for z, _, _ in pairs] == list(range(15))
    for z, j, k in pairs:
        assert ((tj >> 4 * z) & 15, (tk >> 4 * z) & 15) == (j, k), z
    assert tj >> 60 == 0 and tk >> 60 == 0 and tj < 1 << 64 and tk < 1 << 64


# ---------------------------------------------------------------------------------------------------------------------------
def rd(base, q, rev, k=1, mq=60):
    """k rd words: base 0..3 or 4 (N: nt16 code 15), base quality q (the key's quality while q <= mapQ), one strand."""
    nt = 15 if base == 4 else 1 << base
    return np.full(k, q | mq << 8 | nt << 16 | int(rev) << 20 | 20 << 24, dtype=np.int64)


def plain(rng, ref):
    """A cell of one base: 3 to 9 reads of the reference base (A where the reference is N)."""
    k = int(rng.integers(3, 10))
    nt = 1 << (ref if ref < 4 else 0)
    return rng.choice([14, 20, 25, 37], k) | 60 << 8 | nt << 16 | rng.integers(0, 2, k) << 20 | rng.integers(0, 40, k) << 24


def noisy(rng, ref):
    """A cell as sequencing gives them: a few reads of binned qualities, one in ten off the reference base."""
    k = int(rng.poisson(8))
    base = np.where(rng.random(k) < 0.1, rng.integers(0, 4, k), ref if ref < 4 else 0)
    return rng.choice([11, 25, 37, 40], k) | 60 << 8 | (1 << base) << 16 | rng.integers(0, 2, k) << 20 | rng.integers(0, 40, k) << 24


def build(n_smpl, n_sites, special, seed, refs=None, background=plain, shuffle=True):
    """`special`: {cell: function ref -> list of rd arrays}; every other cell is `background`(rng, ref).  refs[s]: the
    reference base of site s, 4 = N (default s % 4)."""
    rng = np.random.default_rng(seed)
    refs = [s % 4 for s in range(n_sites)] if refs is None else list(refs)
    cells = []
    for c in range(n_sites * n_smpl):
        ref = refs[c // n_smpl]
        if c in special:
            r = np.concatenate(special[c](ref))
            if shuffle:
                rng.shuffle(r)
        else:
            r = background(rng, ref)
        cells.append(r)
    off = np.r_[0, np.cumsum([len(c) for c in cells])]
    r = np.concatenate(cells)
    ref16 = np.array([15 if b == 4 else 1 << b for b in refs], dtype=np.int8)
    return host.HostTile(n_smpl, ref16, off.astype(np.uint32), r.astype(np.uint32), rng.integers(0, 100, len(r)).astype(np.uint8))


def check(gpu_ctx_factory, tile, prove, fmt=FMT):
    """The oracle's run, `prove`(want, cr) on it (what the crafted cells must be before they count), then the device's."""
    cfg = abi.default_cfg(tile.n_smpl, max_sites=tile.n_sites, max_reads=len(tile.rd), fmt_flag=fmt)
    want, cr = orc.mpileup(cfg, tile, want_callret=True)
    prove(want, cr)
    got = gpu_ctx_factory(cfg).mpileup(tile)
    assert_mplp_equal(got, want)
    return want, cr


def n_bases(cr, c):
    """Bases with a usable read in cell c: A, C, G, T from the strand counts, the rest of n is N."""
    acgt = cr["ADF"][c].astype(np.int64) + cr["ADR"][c]
    return int((acgt > 0).sum()) + int(int(cr["n"][c]) > int(acgt.sum()))


def assert_not_saturated(want, cr, cells, n_smpl):
    """Over the genotypes of the alleles the cell's site reports: two homozygous likelihoods and one heterozygous one strictly
    between 0 and 250, and the cell has reads of two bases or more."""
    for c in cells:
        s = c // n_smpl
        al = [int(a) for a in want.site["a"][s][:int(want.site["n_alleles"][s])] if 0 <= int(a) < 5]
        p = cr["p"][c].reshape(5, 5)
        hom = [float(p[a, a]) for a in al]
        het = [float(p[a, b]) for i, a in enumerate(al) for b in al[i + 1:]]
        assert n_bases(cr, c) >= 2, (c, cr["ADF"][c], cr["ADR"][c])
        assert sum(0 < x < 250 for x in hom) >= 2, (c, al, hom)
        assert sum(0 < x < 250 for x in het) >= 1, (c, al, het)


def het_cell(rng):
    """Reads of the reference base and of one other, 4 to 9 in all, qualities of 25 and under."""
    kr, ka, d = int(rng.integers(3, 7)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
    qr, qa = int(rng.choice([14, 17, 20, 25])), int(rng.choice([14, 17, 20, 25]))
    return lambda ref: [rd(ref, qr, 1, kr // 2), rd(ref, qr, 0, kr - kr // 2), rd((ref + d) % 4, qa, ka & 1, ka)]


def tile_shape(n_smpl, waves=7):
    """Sites of a tile of `waves` whole wavefronts (448 cells: a second, ragged workgroup); with 4 samples 16 cells more, a
    ragged last wavefront."""
    return waves * 64 // n_smpl + (4 if n_smpl == 4 else 0)


# ---------------------------------------------------------------------------------------------------------------------------
# A: two-base cells

def lanes_of(count):
    return sorted(set([0, 63][:count]) | set(list(range(2, 62, 3))[:max(count - 2, 0)])) if count < 64 else list(range(64))


@gpu
@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_two_base_lanes_per_wavefront(gpu_ctx_factory, n_smpl):
    """Wavefronts with 0, 1, 2, 15, 16 and 64 cells of two bases, one with its only such cell in lane 63; with 4 samples also the
    ragged last wavefront, such cells in its first and in its last lane.  Every other cell has one base."""
    rng = np.random.default_rng(11 + n_smpl)
    n_sites = tile_shape(n_smpl)
    special = {}
    for w, lanes in enumerate([lanes_of(k) for k in (0, 1, 2, 15, 16, 64)] + [[63]]):
        for l in lanes:
            special[w * 64 + l] = het_cell(rng)
    if n_smpl == 4:
        assert n_sites * n_smpl == 464
        special[448], special[463] = het_cell(rng), het_cell(rng)
    assert [sum(w * 64 <= c < w * 64 + 64 for c in special) for w in range(7)] == [0, 1, 2, 15, 16, 64, 1]
    tile = build(n_smpl, n_sites, special, 21 + n_smpl)
    def prove(want, cr):
        assert_not_saturated(want, cr, sorted(special), n_smpl)
        assert all(n_bases(cr, c) <= 1 for c in range(n_sites * n_smpl) if c not in special)
    check(gpu_ctx_factory, tile, prove)


def kinds_of_cells():
    """(function ref -> reads, bases the cell ends up with); ref = 4 at a site whose reference is N."""
    o = lambda ref, d: (ref + d) % 4 if ref < 4 else d % 4               # a base off the reference
    r = lambda ref: ref                                                  # (reads of N where the reference is N)
    return [
        (lambda ref: [rd(r(ref), 20, 1, 2), rd(r(ref), 17, 0, 2), rd(o(ref, 1), 20, 0, 2)], 2),
        (lambda ref: [rd(r(ref), 20, 1, 3), rd(o(ref, 1), 17, 0, 2), rd(o(ref, 2), 14, 1, 1)], 3),
        (lambda ref: [rd(r(ref), 17, 0, 3), rd(o(ref, 1), 17, 0, 1), rd(o(ref, 2), 14, 1, 1), rd(o(ref, 3), 20, 1, 1)], 4),
        (lambda ref: [rd(0, 17, 0, 2), rd(1, 17, 0, 1), rd(2, 14, 1, 1), rd(3, 20, 1, 1), rd(4, 14, 0, 1)], 5),
        (lambda ref: [rd(r(ref) if ref < 4 else 0, 20, 1, 3), rd(4, 17, 0, 2)], 2),                 # reads of N take slot 4
        (lambda ref: [rd(o(ref, 1), 20, 1, 3), rd(o(ref, 2), 17, 0, 2)], 2),                         # no read of the reference base
        (lambda ref: [rd(r(ref) if ref < 4 else 2, 20, 1, 1), rd(o(ref, 3), 17, 0, 1)], 2),          # n = 2
        (lambda ref: [rd(r(ref), 20, 1, 4), rd(o(ref, 1), 11, 0, 2)], 1),                            # the second base under min_baseQ
        (lambda ref: [rd(r(ref), 5, 1, 3), rd(o(ref, 2), 20, 0, 3)], 1),                             # the reference base under it
    ]


@gpu
@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_kinds_of_two_base_cells(gpu_ctx_factory, n_smpl):
    """Cells of 2, 3, 4 and 5 bases, reads of N among them; no read of the reference base; one read each of two bases; cells
    that two bases enter and one is left of after the quality filter (single-base then); every third site with reference N,
    where every read differs.  Every fifth cell is one of them, the rest are ordinary with errors of their own."""
    n_sites = tile_shape(n_smpl)
    refs = [4 if s % 3 == 1 else s % 4 for s in range(n_sites)]
    kinds = kinds_of_cells()
    special, nb = {}, {}
    for i, c in enumerate(range(4, n_sites * n_smpl, 5)):
        # (the stride 5 and the 9 kinds are coprime to the site length's factors: every kind meets every reference, N included)
        special[c], nb[c] = kinds[i % len(kinds)]
    tile = build(n_smpl, n_sites, special, 31 + n_smpl, refs=refs, background=noisy)
    def prove(want, cr):
        for k in range(len(kinds)):
            assert {refs[c // n_smpl] == 4 for i, c in enumerate(sorted(special)) if i % len(kinds) == k} == {False, True}, k
        assert [n_bases(cr, c) for c in sorted(special)] == [nb[c] for c in sorted(special)]
        assert [int(cr["n"][c]) for c in sorted(special)[:9]] == [6, 6, 6, 6, 5, 5, 2, 4, 3]
        assert_not_saturated(want, cr, [c for c in sorted(special) if nb[c] > 1], n_smpl)
    check(gpu_ctx_factory, tile, prove)


@gpu
@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_indel_pass_two_type_cells(gpu_ctx_factory, n_smpl):
    """The indel pass: a read's "base" is its type (p->aux), type 0 the primary one.  Cells of two and of three types among cells
    of type 0 alone."""
    n_sites = tile_shape(n_smpl)
    rng = np.random.default_rng(41 + n_smpl)
    depth = rng.integers(4, 9, n_sites * n_smpl)
    off = np.r_[0, np.cumsum(depth)]
    R = int(off[-1])
    cell = np.repeat(np.arange(n_sites * n_smpl), depth)
    k_in = np.arange(R) - off[cell]                                      # a read's place in its cell
    crafted = np.arange(3, n_sites * n_smpl, 7)
    three = crafted[::2]
    typ = np.zeros(R, np.int64)
    in_c, in_3 = np.isin(cell, crafted), np.isin(cell, three)
    typ[in_c & (k_in < 2)] = 1 + cell[in_c & (k_in < 2)] % 3             # two reads of another type at the head of the cell
    typ[in_3 & (k_in == depth[cell] - 1)] = 1 + (cell[in_3 & (k_in == depth[cell] - 1)] + 1) % 3     # a third type as the last read
    base_q = np.where(in_c, rng.choice([14, 17, 20], R), rng.choice([5, 20, 40], R))
    aux = typ << 16 | rng.choice([30, 45, 60], R) << 8 | base_q
    rdw = rng.choice([14, 20, 25], R) | 60 << 8 | (1 << (cell // n_smpl % 4)) << 16 | rng.integers(0, 2, R) << 20 | rng.integers(0, 40, R) << 24
    tile = host.HostTile(n_smpl, (1 << (np.arange(n_sites) % 4)).astype(np.int8), off.astype(np.uint32), rdw.astype(np.uint32),
                         rng.integers(0, 100, R).astype(np.uint8), aux=aux.astype(np.uint32), is_indel=1)
    cfg = abi.default_cfg(n_smpl, max_sites=n_sites, max_reads=R, fmt_flag=abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD)
    want, cr = orc.mpileup(cfg, tile, want_callret=True)
    live = want.site["ret"] == 0
    assert live[crafted // n_smpl].all()
    assert_not_saturated(want, cr, crafted.tolist(), n_smpl)
    assert {n_bases(cr, c) for c in three.tolist()} == {3} and {n_bases(cr, c) for c in crafted[1::2].tolist()} == {2}
    got = gpu_ctx_factory(cfg).mpileup(tile)
    np.testing.assert_array_equal(got.site["ret"], want.site["ret"])
    for k in EXACT_SITE:
        np.testing.assert_array_equal(got.site[k][live], want.site[k][live], err_msg="site." + k)
    for k in ["pl", "dp4", "adf", "adr"]:
        np.testing.assert_array_equal(getattr(got, k)[live], getattr(want, k)[live], err_msg=k)
    for k in FLOAT_SITE:
        g, w = got.site[k][live].astype(np.float64), want.site[k][live].astype(np.float64)
        assert np.array_equal(np.isinf(g), np.isinf(w)), k
        m = ~np.isinf(w)
        np.testing.assert_allclose(g[m], w[m], rtol=2e-6, atol=1e-30, err_msg=k)


GLF_MAX_WINDOW = 16384            # csrc/kernels.h: the most keys a workgroup's LDS window ever holds


@gpu
@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_listed_deep_cell_of_two_bases(gpu_ctx_factory, n_smpl):
    """A cell of 17 000 pileup entries is listed for the launch that gives it a workgroup of its own; about one entry in a
    thousand passes min_baseQ, four in ten of those off the reference base: its 15 likelihoods come from the one wavefront of
    that workgroup that holds the cell."""
    rng = np.random.default_rng(51 + n_smpl)
    n_sites = 2 if n_smpl == 64 else 12
    depths = rng.poisson(8, n_sites * n_smpl).astype(np.int64)
    deep = n_smpl + 1
    depths[deep] = 17000
    assert depths[deep] > GLF_MAX_WINDOW - 3
    R = int(depths.sum())
    cell = np.repeat(np.arange(n_sites * n_smpl), depths)
    ref = (cell // n_smpl) % 4
    in_deep = cell == deep
    bq = np.where(in_deep, np.where(rng.random(R) < 0.001, rng.choice([14, 17, 20], R), 5), rng.choice([11, 25, 37, 40], R))
    base = np.where(rng.random(R) < np.where(in_deep, 0.4, 0.1), (ref + 1 + rng.integers(0, 2, R)) % 4, ref)
    rdw = bq | 60 << 8 | (1 << base) << 16 | rng.integers(0, 2, R) << 20 | rng.integers(0, 40, R) << 24
    tile = host.HostTile(n_smpl, (1 << (np.arange(n_sites) % 4)).astype(np.int8), np.r_[0, np.cumsum(depths)].astype(np.uint32),
                         rdw.astype(np.uint32), rng.integers(0, 100, R).astype(np.uint8))
    def prove(want, cr):
        assert 4 <= int(cr["n"][deep]) < 64 and int(cr["n"][deep]) == int((in_deep & (bq >= 13)).sum())
        assert_not_saturated(want, cr, [deep], n_smpl)
    check(gpu_ctx_factory, tile, prove)


@gpu
@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_cell_past_255_reads_of_two_bases(gpu_ctx_factory, n_smpl):
    """300 usable reads of the lowest quality (a mapQ of 4 caps the key's), two bases in turn: errmod_cal sees the first 255, the counts are of all 300.  (A
    balanced heterozygote of 255 reads is the one genotype of such a cell whose likelihood stays under PL's 255.)"""
    def deep2(ref):
        return [np.stack([rd(ref, 20, 1, 75, 4), rd((ref + 1) % 4, 20, 0, 75, 4), rd(ref, 20, 0, 75, 4), rd((ref + 1) % 4, 20, 1, 75, 4)], axis=1).ravel()]
    n_sites = tile_shape(n_smpl, waves=5)
    special = {70: deep2, 300: deep2}
    tile = build(n_smpl, n_sites, special, 61 + n_smpl, background=noisy, shuffle=False)
    def prove(want, cr):
        assert [int(cr["n"][c]) for c in sorted(special)] == [300, 300]
        assert_not_saturated(want, cr, sorted(special), n_smpl)
    check(gpu_ctx_factory, tile, prove, FMT | abi.FMT_DP4)


# ---------------------------------------------------------------------------------------------------------------------------
# B: the other bases

def one_other(where, q_other, d):
    """Five reads of the reference base at quality 20 and one of another base: the cell's first, middle or last read, with a
    quality under or above the others'."""
    def f(ref):
        a, b = {"first": (0, 5), "middle": (3, 2), "last": (5, 0)}[where]
        return [rd(ref, 20, 1, a), rd((ref + 1 + d % 3) % 4, q_other, d & 1, 1), rd(ref, 20, 0, b)]
    return f


ONE_OTHER = [one_other(w, q, d) for d, (w, q) in enumerate([(w, q) for w in ("first", "middle", "last") for q in (14, 25)], 1)]
TWO_DIFF = lambda ref: [rd(ref, 20, 1, 2), rd((ref + 1) % 4, 17, 0, 1), rd(ref, 20, 0, 2), rd((ref + 2) % 4, 14, 1, 1)]
TWO_SAME = lambda ref: [rd((ref + 3) % 4, 17, 0, 1), rd(ref, 20, 1, 4), rd((ref + 3) % 4, 14, 1, 1)]


@gpu
@pytest.mark.parametrize("layout", ["one", "two_diff", "two_same", "mix"])
@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_other_bases(gpu_ctx_factory, n_smpl, layout):
    """"one": no cell of the tile has two reads off its primary base, every wavefront but the first (which has none at all)
    takes the one-product path.  "two_diff" / "two_same": every wavefront also holds a cell with two such reads, of two bases /
    of one base, and takes the loop over bases -- its form without a walk / with the walk.  "mix": the three kinds of wavefront in
    turn."""
    n_sites = tile_shape(n_smpl)
    n_cells = n_sites * n_smpl
    special, twos = {}, []
    for w in range(1, -(-n_cells // 64)):
        lanes = [l for l in (0, 5, 17, 30, 31, 32, 47, 63) if w * 64 + l < n_cells]
        for i, l in enumerate(lanes):
            special[w * 64 + l] = ONE_OTHER[(i + w) % len(ONE_OTHER)]
        kind = {"one": None, "two_diff": TWO_DIFF, "two_same": TWO_SAME, "mix": (None, TWO_DIFF, TWO_SAME)[w % 3]}[layout]
        if kind is not None:
            special[w * 64 + lanes[w % len(lanes)] + 1 - 2 * (lanes[w % len(lanes)] == 63)] = kind
            twos.append(w)
    tile = build(n_smpl, n_sites, special, 71 + n_smpl, shuffle=False)
    def prove(want, cr):
        assert_not_saturated(want, cr, sorted(special), n_smpl)
        assert all(n_bases(cr, c) == 1 for c in range(n_cells) if c not in special)
        off_ref = [int(cr["n"][c]) - int(cr["ADF"][c][c // n_smpl % 4]) - int(cr["ADR"][c][c // n_smpl % 4]) for c in range(n_cells)]
        assert {w for w in range(-(-n_cells // 64)) if max(off_ref[w * 64:w * 64 + 64]) > 1} == set(twos)
        assert max(off_ref[:64]) == 0 and all(max(off_ref[w * 64:w * 64 + 64]) >= 1 for w in range(1, -(-n_cells // 64)))
        assert bool(twos) == (layout != "one") and (layout != "mix" or len(twos) < -(-n_cells // 64) - 1)
    check(gpu_ctx_factory, tile, prove)
