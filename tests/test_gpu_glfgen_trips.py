"""glfgen_kernel's phase A by the geometry of a site segment, against the oracle.

A wavefront's trip covers 256 consecutive reads, the next trip of the same wavefront lies 1024 reads on.  A trip whose reads
all lie inside the segment [rb, re) is a full trip: full trips run in a loop of their own (no byte mask, 8-byte key stores,
unguarded loads from a scalar base), provided the loads for the trip behind it stay inside the tile's arrays; every other
trip -- the ragged ends of a segment, the tile's last reads -- runs the general body.  So the tiles here are chosen by where
the ends of a segment fall, not by size: segment lengths on both sides of the first full trip and of the ones behind it, for
each wavefront and each alignment of the segment's start; segments that meet inside a wavefront's block; tiles that end
inside or just behind a full trip's loads; and the forms that share the code (the global-histogram form, the indel pass, no
epos loads, the launch for a listed deep cell).

Every test compares all mpileup planes and the site records, as tests/test_gpu_glfgen_fields.py does."""
import numpy as np
import pytest

from bcftools_amd import abi, host
from tests.helpers import orc
from tests.helpers import sitestats as ss
from tests.test_gpu_parity import assert_mplp_equal

pytestmark = pytest.mark.gpu

FMT_ALL = abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD | abi.FMT_QS | abi.FMT_SCR | abi.INFO_SCR | abi.FMT_SP
MIN_BASEQ = 13


def spread(total, cells):
    """`total` reads over `cells` cells, as evenly as they go (the first cells take the remainder)."""
    d = np.full(cells, total // cells, np.int64)
    d[:total % cells] += 1
    return d


def tile_of_depths(seed, n_smpl, depths, indel=False):
    """A tile with the given per-cell depths (sites x n_smpl, flattened) and reads whose fields take edge values often: the
    planes of a full trip and of a general trip must agree on every one of them."""
    rng = np.random.default_rng(seed)
    depths = np.asarray(depths, np.int64).ravel()
    n_sites = len(depths) // n_smpl
    assert n_sites * n_smpl == len(depths)
    off = np.r_[0, np.cumsum(depths)]
    n = int(off[-1])
    ref2 = rng.integers(0, 4, n_sites)
    ref16 = np.where(rng.random(n_sites) < 0.1, 15, 1 << ref2).astype(np.int8)
    site = np.repeat(np.arange(n_sites), depths.reshape(n_sites, n_smpl).sum(1))
    bq = rng.choice([2, 11, MIN_BASEQ - 1, MIN_BASEQ, 25, 37, 40, 41, 59, 60, 93], n)
    mq = np.where(rng.random(n) < 0.8, 60, rng.choice([0, 1, 19, 20, 58, 59, 61, 254, 255], n))
    base = np.where(rng.random(n) < 0.9, ref2[site], rng.integers(0, 4, n))
    nt = np.where(rng.random(n) < 0.03, rng.integers(0, 16, n), 1 << base)
    flags = rng.integers(0, 2, n) | (rng.random(n) < 0.05).astype(np.int64) << 1              # strand, soft clip
    u = rng.random(n)
    extra = np.where(u < 0.02, abi.RD_SKIP, np.where(u < 0.04, abi.RD_DEL, np.where(u < 0.045, abi.RD_SKIP | abi.RD_DEL, 0)))
    tail = np.where(rng.random(n) < 0.2, rng.choice([0, 1, 24, 25, 26, 255], n), rng.integers(0, 75, n))
    rd = (bq | mq << 8 | nt << 16 | flags << 20 | extra | tail << 24).astype(np.uint32)
    epos = rng.integers(0, 100, n).astype(np.uint8)
    if not indel:
        return host.HostTile(n_smpl, ref16, off.astype(np.uint32), rd, epos)
    rd = (rd.astype(np.int64) & ~np.int64(abi.RD_DEL)).astype(np.uint32)      # (deletions are not an indel-pass filter)
    abq = rng.choice([0, MIN_BASEQ - 1, MIN_BASEQ, 30, 40, 93], n)
    asq = rng.choice([0, 12, 13, 20, 60, 255], n)
    aux = (abq | asq << 8 | rng.integers(0, 5, n) << 16).astype(np.uint32)
    return host.HostTile(n_smpl, np.zeros(n_sites, np.int8), off.astype(np.uint32), rd, epos, aux=aux, is_indel=1)


def segments(n_smpl, lengths, start_mod4):
    """Per-cell depths of one site per entry of `lengths`, each behind a filler site of a few reads that puts the site's
    first read at `start_mod4` modulo 4."""
    out, at = [], 0
    for r in lengths:
        fill = (start_mod4 - at) % 4 + 4
        out += [spread(fill, n_smpl), spread(r, n_smpl)]
        at += fill
        assert at % 4 == start_mod4
        at += r
    return np.concatenate(out)


def check(gpu_ctx_factory, tile, fmt=FMT_ALL):
    cfg = abi.default_cfg(tile.n_smpl, max_sites=tile.n_sites, max_reads=len(tile.rd), fmt_flag=fmt, min_baseQ=MIN_BASEQ)
    want = orc.mpileup(cfg, tile)
    got = gpu_ctx_factory(cfg).mpileup(tile)
    # A statistic that was not asked for has no value: the oracle leaves HUGE_VAL in its field, combine_kernel 0 (it is the
    # same in every tile, whatever phase A did).  Every field that has a value is compared.
    for flag, k in ((abi.INFO_VDB, "vdb"), (abi.INFO_RPB, "mwu_pos")):
        if not fmt & flag:
            assert np.isinf(want.site[k]).all() and (got.site[k] == 0).all(), k
            want.site[k] = got.site[k]
    assert_mplp_equal(got, want)
    assert (want.site["anno"] != 0).any()
    return got, want


# One site a workgroup (256 samples).  Wavefront w's trip t starts 1024 t + 256 w reads behind the segment's start rounded
# down to 4: its first full trip appears at 256 (w + 1) reads (one trip later for wavefront 0 when the start is not a
# multiple of 4), the next one 1024 reads later, and a segment of 3 x 1024 or 8 x 1024 reads holds an odd or an even count
# of full trips depending on the wavefront and the alignment (a loop that took them in pairs would have to get both right).
LENGTHS = [1023, 1024, 1025, 2047, 2049, 3072, 3073, 3 * 1024 + 255, 3 * 1024 + 257, 8 * 1024 - 1, 8 * 1024 + 3]


@pytest.mark.parametrize("start_mod4", [0, 1, 2, 3])
def test_segment_lengths(gpu_ctx_factory, start_mod4):
    """Every length beside every alignment of the segment's start; the sites behind a segment keep its full trips' loads
    inside the tile (the last, longest segment has the tile's end behind it: its last trips run as general trips)."""
    tile = tile_of_depths(100 + start_mod4, 256, segments(256, LENGTHS, start_mod4))
    sites = np.diff(tile.plp_off.astype(np.int64)[::256])
    assert list(sites[1::2]) == LENGTHS and all(int(o) % 4 == start_mod4 for o in tile.plp_off[256::512])
    check(gpu_ctx_factory, tile)


@pytest.mark.parametrize("n_smpl,n_sites,depth,seed", [
    (100, 8, 30, 111),                  # four histogram slots: 2.56 sites a workgroup, segments of 3000 reads and shorter
    (1000, 2, 12, 112),                 # the site boundary inside the fourth workgroup, inside a wavefront's block
])
def test_two_segments_in_a_workgroup(gpu_ctx_factory, n_smpl, n_sites, depth, seed):
    rng = np.random.default_rng(seed)
    depths = np.minimum(rng.poisson(depth, n_sites * n_smpl), 200)
    depths[n_smpl - 1] += 1 + (-int(depths[:n_smpl].sum())) % 2        # the second site starts at an odd read
    tile = tile_of_depths(seed, n_smpl, depths)
    assert int(tile.plp_off[n_smpl]) % 2 == 1
    check(gpu_ctx_factory, tile)


# The tile's end.  The last site is the last workgroup; a full trip at `first` needs first + 1280 <= n_reads (the loads for
# the trip behind it).  With the segment starting at a multiple of 4, wavefront 0's trips start at 0, 1024, 2048, ...,
# wavefront 3's at 768, 1792, ...: lengths on both sides of 1280, 2048 (wavefront 3), 2304, 3072 and 4352, and lengths that
# leave 1, 2 or 3 reads behind the last whole quad.
@pytest.mark.parametrize("last,start_mod4", [
    (1279, 0), (1280, 0), (1281, 0), (1282, 1), (2047, 0), (2048, 0), (2049, 3),
    (2303, 0), (2304, 0), (2305, 1), (2306, 2), (2307, 3),
    (3071, 0), (3072, 0), (3073, 0), (3074, 3),
    (4351, 0), (4352, 0), (4353, 0), (4354, 1), (4355, 2),
    (6 * 1024 + 2, 0), (6 * 1024 + 259, 2),
])
def test_tile_end(gpu_ctx_factory, last, start_mod4):
    tile = tile_of_depths(200 + last, 256, segments(256, [last], start_mod4))
    assert len(tile.rd) == int(tile.plp_off[-1]) and len(tile.rd) == 4 + start_mod4 + last
    check(gpu_ctx_factory, tile)


def test_global_histogram_form(gpu_ctx_factory):
    """8 samples: 32 sites a workgroup, every segment far shorter than a wavefront's block -- no full trip."""
    rng = np.random.default_rng(121)
    tile = tile_of_depths(121, 8, np.minimum(rng.poisson(20, 300 * 8), 200))
    check(gpu_ctx_factory, tile)


def test_global_histogram_form_with_full_trips(gpu_ctx_factory):
    """8 samples at depth: segments of 1600 reads, so the global-atomic instantiation runs its full trips too."""
    rng = np.random.default_rng(122)
    tile = tile_of_depths(122, 8, np.minimum(rng.poisson(190, 40 * 8), 200))
    check(gpu_ctx_factory, tile)


@pytest.mark.parametrize("start_mod4", [0, 3])
def test_indel_tile(gpu_ctx_factory, start_mod4):
    """The indel pass loads the aux words beside the rd words, in full trips as well."""
    tile = tile_of_depths(130 + start_mod4, 256, segments(256, [2049, 3073, 5 * 1024 + 7, 2500], start_mod4), indel=True)
    check(gpu_ctx_factory, tile, fmt=abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD)


@pytest.mark.parametrize("start_mod4", [0, 2])
def test_without_epos(gpu_ctx_factory, start_mod4):
    """Neither RPB nor VDB asked for: no epos loads, in either loop."""
    tile = tile_of_depths(140 + start_mod4, 256, segments(256, [2049, 3073, 5 * 1024 + 7, 2500], start_mod4))
    check(gpu_ctx_factory, tile, fmt=abi.FMT_AD | abi.FMT_QS | abi.FMT_SP | abi.FMT_SCR | abi.INFO_SCR)


DEEP_CELL, DEEP_READS = 5, 20003        # more reads than the largest key window (16 384): the cell is listed


def deep_cell_tile(seed=150):
    """37 samples, one site: cell 5 with 20 003 reads (a workgroup of its own works on it, nearly all its trips full), the
    other cells at depth 12.  The reads are made as tests/helpers/sitestats.py makes its listed cell's: every read accepted,
    so that the numpy twin applies."""
    rng = np.random.default_rng(seed)
    cells = []
    for i in range(37):
        n = DEEP_READS if i == DEEP_CELL else 12
        alt = rng.random(n) < (0.04 if i == DEEP_CELL else 0.3)
        odd = alt | (rng.random(n) < 0.05)
        bq = np.where(odd, rng.choice([20, 30, 37, 40], n), 40)
        mq = np.where(odd, rng.choice([20, 40, 60], n), 60)
        ep = np.where(odd, rng.integers(0, 100, n), 50)
        cells.append((ss._pack(bq, mq, np.where(alt, ss.NT_C, ss.NT_A), rng.integers(0, 2, n)), ep))
    off = np.r_[0, np.cumsum([len(c[0]) for c in cells])]
    return host.HostTile(37, np.array([ss.NT_A], np.int8), off.astype(np.uint32), np.concatenate([c[0] for c in cells]),
                         np.concatenate([c[1] for c in cells]).astype(np.uint8))


def test_listed_deep_cell(gpu_ctx_factory):
    """The conditions of tests/test_gpu_site_stats.py for a listed cell: the oracle's planes and records, and the numpy twin
    of the site's statistics and of FMT/SP."""
    tile = deep_cell_tile()
    cfg = ss.make_cfg(tile)
    want = orc.mpileup(cfg, tile)
    got = gpu_ctx_factory(cfg).mpileup(tile)
    assert_mplp_equal(got, want)
    tw = ss.twin_stats(tile)
    for k in ss.STATS:
        g, w = got.site[k].astype(np.float64), tw[k].astype(np.float64)
        assert np.array_equal(np.isinf(g), np.isinf(w)), k
        m = ~np.isinf(w)
        np.testing.assert_allclose(g[m], w[m], rtol=ss.RTOL, atol=ss.ATOL, err_msg="twin " + k)
    np.testing.assert_array_equal(got.sp, ss.twin_sp(tile), err_msg="twin sp")
