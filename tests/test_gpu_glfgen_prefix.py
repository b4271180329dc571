"""glfgen_kernel's errmod walk starts from the context's prefix table: the double sum after a cell's highest quality is
looked up by (quality, n, reverse-strand reads, forward-strand reads) when n < 64 and both counts are below 32, and walked
read by read otherwise.  Crafted cells on both sides of every bound of that domain, and on every path that enters the walk
(primary base, the other bases' general path, a second round of qualities, the indel pass, the launch for listed deep cells),
compared field by field and bit for bit with the oracle -- in a tile of 64 samples (histograms in LDS) and in one of 4 (global
histograms).  The special cells sit among ordinary ones, so that a wavefront holds lanes that take the table and lanes that
do not."""
import numpy as np
import pytest

from bcftools_amd import abi, synth, host
from tests.helpers import orc
from tests.test_gpu_parity import assert_mplp_equal, EXACT_SITE, FLOAT_SITE

pytestmark = pytest.mark.gpu

FMT = abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD | abi.FMT_QS | abi.FMT_SP
SAMPLES = [64, 4]                 # hist_slots > 0 (n_smpl >= 37) and the global-histogram form


def reads(base, q, rev, k, mq=60):
    """k rd words: base quality q (the key's quality while q <= mapQ), one base, one strand."""
    return np.full(k, q | mq << 8 | (1 << base) << 16 | int(rev) << 20 | 20 << 24, dtype=np.int64)


def ordinary(rng, ref):
    """A cell as sequencing gives them: a dozen reads of four binned qualities, one in ten off the reference base."""
    k = int(rng.poisson(12))
    base = np.where(rng.random(k) < 0.1, rng.integers(0, 4, k), ref)
    return (rng.choice([11, 25, 37, 40], k) | 60 << 8 | (1 << base) << 16 | rng.integers(0, 2, k) << 20 | rng.integers(0, 40, k) << 24)


def tile_with(n_smpl, special, seed, every=5, shuffle=True):
    """`special`: functions ref -> list of rd arrays, one cell each.  They take every `every`-th cell of the tile, ordinary cells
    the rest; site s has reference base s % 4."""
    rng = np.random.default_rng(seed)
    n_cells = -(-len(special) * every // n_smpl) * n_smpl
    cells, where = [], []
    for c in range(n_cells):
        ref = (c // n_smpl) % 4
        if c % every == every - 1 and c // every < len(special):
            rd = np.concatenate(special[c // every](ref))
            if shuffle:
                rng.shuffle(rd)
            where.append(c)
        else:
            rd = ordinary(rng, ref)
        cells.append(rd)
    assert len(where) == len(special)
    off = np.r_[0, np.cumsum([len(c) for c in cells])]
    rd = np.concatenate(cells)
    n_sites = n_cells // n_smpl
    ref16 = (1 << (np.arange(n_sites) % 4)).astype(np.int8)
    return host.HostTile(n_smpl, ref16, off.astype(np.uint32), rd.astype(np.uint32), rng.integers(0, 100, len(rd)).astype(np.uint8)), where


def check(gpu_ctx_factory, tile, fmt=FMT):
    cfg = abi.default_cfg(tile.n_smpl, max_sites=tile.n_sites, max_reads=len(tile.rd), fmt_flag=fmt)
    want, cr = orc.mpileup(cfg, tile, want_callret=True)
    got = gpu_ctx_factory(cfg).mpileup(tile)
    assert_mplp_equal(got, want)
    return want, cr


def assert_sums_show(cr, cells):
    """The double sum of a single-base cell reaches the outputs as the PL of the genotypes without that base, and PL stops at
    255: the crafted cells keep their sums under it, so that a wrong sum is a wrong PL."""
    for c in cells:
        a = cr["p"][c].reshape(5, 5).diagonal().max()
        assert 0 < a < 250, (c, a)


@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_whole_cell_from_the_table(gpu_ctx_factory, n_smpl):
    """Cells whose reads are all of one quality: the table holds the whole sum and no step of the walk is left.  Reverse strand
    only, forward only, both; one read; and the same at the lowest (4: a mapQ under it) and the highest (60) key quality."""
    special = []
    for q, mq, k in ((40, 60, 2), (37, 60, 2), (13, 60, 5), (60, 60, 1), (30, 2, 5)):     # (fewer reads at the high qualities: PL < 255)
        special += [lambda ref, q=q, mq=mq, k=k: [reads(ref, q, 1, k + 2, mq)],
                    lambda ref, q=q, mq=mq, k=k: [reads(ref, q, 0, k + 3, mq)],
                    lambda ref, q=q, mq=mq, k=k: [reads(ref, q, 1, k, mq), reads(ref, q, 0, k + 1, mq)],
                    lambda ref, q=q, mq=mq, k=k: [reads(ref, q, 0, 1, mq)]]
    tile, where = tile_with(n_smpl, special, 101 + n_smpl)
    want, cr = check(gpu_ctx_factory, tile)
    assert [int(cr["n"][c]) for c in where[:4]] == [4, 5, 5, 1]
    assert_sums_show(cr, where)


@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_edges_of_the_table(gpu_ctx_factory, n_smpl):
    """31 reads of the top quality on a strand are inside the table, 32 are not; a cell of 63 reads is inside, one of 64 is not
    (there the top quality is a single read, so that only n decides).  31 + 31 reads in a cell of 63 is the table's last row.
    Low qualities keep every sum under PL's 255."""
    low = lambda ref, k: [reads(ref, 14, 1, k // 2), reads(ref, 14, 0, k - k // 2)]
    special = []
    for k in (31, 32):
        special += [lambda ref, k=k: [reads(ref, 20, 1, k)] + low(ref, 5),                      # reverse strand at the edge
                    lambda ref, k=k: [reads(ref, 20, 0, k)] + low(ref, 5),                      # forward strand
                    lambda ref, k=k: [reads(ref, 20, 1, k), reads(ref, 20, 0, 3)] + low(ref, 4),
                    lambda ref, k=k: [reads(ref, 20, 1, 3), reads(ref, 20, 0, k)] + low(ref, 4),
                    lambda ref, k=k: [reads(ref, 20, 1, k), reads(ref, 20, 0, k)]]                # 62 and 64 reads, nothing else
    special.append(lambda ref: [reads(ref, 20, 1, 31), reads(ref, 20, 0, 31), reads(ref, 14, 0, 1)])      # n = 63
    special.append(lambda ref: [reads(ref, 20, 1, 31), reads(ref, 20, 0, 31), reads(ref, 14, 0, 2)])      # n = 64
    for n in (62, 63, 64, 65):
        special += [lambda ref, n=n: [reads(ref, 41, 1, 1)] + low(ref, n - 1),
                    lambda ref, n=n: [reads(ref, 41, 0, 1)] + low(ref, n - 1),
                    # n counts the reads of every base: the reference base alone stays under 64
                    lambda ref, n=n: [reads(ref, 41, 1, 1)] + low(ref, n - 4) + [reads((ref + 1) % 4, 14, 0, 3)]]
    tile, where = tile_with(n_smpl, special, 202 + n_smpl)
    want, cr = check(gpu_ctx_factory, tile)
    ns = [int(cr["n"][c]) for c in where]
    assert ns[10:12] == [63, 64] and ns[12::3] == [62, 63, 64, 65]
    assert_sums_show(cr, [c for i, c in enumerate(where) if i < 12 or i % 3 != 2])     # (the single-base cells)


@pytest.mark.parametrize("n_sites,n_smpl,depth", [(6, 64, 45.0), (40, 4, 45.0)])
def test_more_qualities_than_a_round_takes(gpu_ctx_factory, n_sites, n_smpl, depth):
    """Unbinned qualities: cells with more distinct qualities than a round counts (NRANK, 10) go round again, and only the
    first round starts from the table; the later ones go on from the sum they find."""
    tile = synth.numpy_tile(303 + n_smpl, n_sites, n_smpl, depth=depth, var_rate=0.4, wide_qual=True)
    off = tile.plp_off.astype(np.int64)
    # every third cell keeps three binned qualities and mapQ 60: lanes of one and of several rounds in a wavefront
    rng = np.random.default_rng(n_smpl)
    binned = np.repeat(np.arange(len(off) - 1) % 3 == 0, np.diff(off))
    tile.rd[binned] = (tile.rd[binned] & ~np.uint32(0xffff)) | rng.choice([25, 37, 40], int(binned.sum())).astype(np.uint32) | np.uint32(60 << 8)
    bq, mq = (tile.rd & 0xff).astype(np.int64), (tile.rd >> 8 & 0xff).astype(np.int64)
    q = np.where(bq >= 13, np.clip(np.minimum(bq, mq), 4, 63), 0)             # the key's quality, 0: not a read
    nq = [len(set(q[a:b].tolist()) - {0}) for a, b in zip(off[:-1], off[1:])]
    assert min(nq) <= 3 and sum(10 < k <= 20 for k in nq) and max(nq) > 20  # one, two and three rounds in the tile
    check(gpu_ctx_factory, tile)


@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_other_bases_general_path(gpu_ctx_factory, n_smpl):
    """Two or more reads of a base that is not the primary one send the wavefront down walk_runs for that base: its top quality
    with reads on both strands, on one strand, at the table's edge, and of several bases in one cell."""
    def het(k_ref, alt_groups):
        return lambda ref: [reads(ref, 40, 1, k_ref // 2), reads(ref, 40, 0, k_ref - k_ref // 2), reads(ref, 25, 1, 2)] + \
                           [reads((ref + d) % 4, q, rev, k) for d, q, rev, k in alt_groups]
    special = [het(10, [(1, 37, 1, 2), (1, 37, 0, 3), (1, 25, 0, 1)]),
               het(8, [(2, 40, 1, 4), (2, 11, 0, 2)]),                      # (quality 11: under min_baseQ, not a read)
               het(6, [(1, 41, 0, 2), (1, 40, 1, 5), (3, 37, 1, 1), (3, 37, 0, 1)]),
               het(4, [(1, 14, 1, 31), (1, 14, 0, 2)]),                        # (low quality: the base's sum stays under PL's 255)
               het(4, [(1, 14, 1, 32), (1, 14, 0, 2)]),
               het(20, [(1, 14, 1, 20), (1, 14, 0, 21), (2, 25, 0, 2)]),    # n = 65: no base of the cell takes the table
               lambda ref: [reads((ref + 1) % 4, 40, 1, 6), reads((ref + 1) % 4, 40, 0, 5)]]      # no read of the primary base
    tile, where = tile_with(n_smpl, special * 2, 404 + n_smpl, every=3)
    want, cr = check(gpu_ctx_factory, tile)
    assert (want.sp > 0).any()


@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_over_deep_cell_takes_no_table(gpu_ctx_factory, n_smpl):
    """300 usable reads: errmod_cal sees the first 255 (n = 255, outside the table) whatever the top quality's counts are -- here
    3 reads at the head of the cell."""
    special = [lambda ref: [reads(ref, 41, 1, 2), reads(ref, 41, 0, 1), reads(ref, 37, 1, 150), reads(ref, 25, 0, 147)],
               lambda ref: [reads(ref, 40, 1, 150), reads(ref, 40, 0, 150)]]
    tile, where = tile_with(n_smpl, special, 505 + n_smpl, shuffle=False)
    want, cr = check(gpu_ctx_factory, tile, FMT | abi.FMT_DP4)
    assert [int(cr["n"][c]) for c in where] == [300, 300]


@pytest.mark.parametrize("n_sites,n_smpl", [(8, 64), (48, 4)])
def test_indel_pass(gpu_ctx_factory, n_sites, n_smpl):
    """The indel pass (types and qualities from p->aux, primary type 0) walks with the same start."""
    seed = 606 + n_smpl
    base = synth.numpy_tile(seed, n_sites, n_smpl, depth=20.0, var_rate=0.0)
    rng = np.random.default_rng(seed)
    R = len(base.rd)
    cell = np.repeat(np.arange(n_sites * n_smpl), np.diff(base.plp_off.astype(np.int64)))
    has_indel = rng.random(n_sites) < 0.8
    carrier = rng.random(n_sites * n_smpl) < 0.4
    typ = np.where(has_indel[cell // n_smpl] & carrier[cell] & (rng.random(R) < 0.5), rng.integers(1, 4, R), 0)
    aux = typ.astype(np.uint32) << 16 | rng.choice([30, 45, 60, 200], R).astype(np.uint32) << 8 | rng.choice([5, 20, 40, 60], R).astype(np.uint32)
    tile = host.HostTile(n_smpl, base.ref16, base.plp_off, base.rd, base.epos, aux=aux, is_indel=1)
    cfg = abi.default_cfg(n_smpl, max_sites=n_sites, max_reads=R, fmt_flag=abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD)
    want = orc.mpileup(cfg, tile)
    got = gpu_ctx_factory(cfg).mpileup(tile)
    np.testing.assert_array_equal(got.site["ret"], want.site["ret"])
    live = want.site["ret"] == 0
    assert live.sum() >= 3
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


@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_listed_deep_cell(gpu_ctx_factory, n_smpl):
    """A cell of 17 000 pileup entries.  The tile launch lists a cell of more than window - 3 entries for the launch that gives
    each listed cell a workgroup of its own (DEEP), and csrc/api.hip sizes the window from the tile's mean depth but never above
    GLF_MAX_WINDOW keys: this cell is listed whatever window the tile gets.  About one entry in a thousand passes min_baseQ,
    all of the reference base and of low quality, so the cell is inside the table, its walk in the DEEP launch starts from
    an entry, and its sum stays under PL's 255."""
    rng = np.random.default_rng(707 + n_smpl)
    n_sites = 2 if n_smpl == 64 else 12
    depths = rng.poisson(12, n_sites * n_smpl).astype(np.int64)
    deep = n_smpl + 1
    depths[deep] = 17000
    assert depths[deep] > GLF_MAX_WINDOW - 3                                # listed at the largest window
    R = int(depths.sum())
    cell = np.repeat(np.arange(n_sites * n_smpl), depths)
    ref = (cell // n_smpl) % 4
    in_deep = cell == deep
    bq = np.where(in_deep, np.where(rng.random(R) < 0.001, rng.choice([14, 17, 20], R), 5), rng.choice([11, 25, 37, 40], R))
    base = np.where(~in_deep & (rng.random(R) < 0.1), rng.integers(0, 4, R), ref)
    strand = rng.integers(0, 2, R)
    rd = bq | 60 << 8 | (1 << base) << 16 | strand << 20 | rng.integers(0, 40, R) << 24
    tile = host.HostTile(n_smpl, (1 << (np.arange(n_sites) % 4)).astype(np.int8), np.r_[0, np.cumsum(depths)].astype(np.uint32),
                         rd.astype(np.uint32), rng.integers(0, 100, R).astype(np.uint8))
    # inside the table: n < 64, and the top quality has reads, fewer than 32 on either strand
    top = in_deep & (bq == bq[in_deep].max())
    n_rev, n_fwd = int((top & (strand == 1)).sum()), int((top & (strand == 0)).sum())
    assert bq[in_deep].max() >= 14 and 0 < n_rev + n_fwd and n_rev < 32 and n_fwd < 32
    want, cr = check(gpu_ctx_factory, tile)
    assert 2 <= int(cr["n"][deep]) < 64 and int(cr["n"][deep]) == int((in_deep & (bq >= 13)).sum())
    assert_sums_show(cr, [deep])


def walk_sum(groups, n):
    """errmod_cal's double sum for one base: `groups` = (quality, reverse reads, forward reads) from the highest quality down, a
    multiply and an add per read in the reference's order, from the oracle's own fk and beta (beta[q << 16 | n << 8 | k])."""
    L = orc.lib()
    em = L.orc_errmod_init(1.0 - 0.83)
    try:
        fk = np.ctypeslib.as_array(L.orc_errmod_fk(em), (256,)).copy()
        beta = np.ctypeslib.as_array(L.orc_errmod_beta(em), (64 * 256 * 256,))
        bs, k, w = np.float64(0.0), 0, [0, 0]                     # reads so far: all, per strand
        for q, nr, nf in groups:
            for strand, cnt in ((0, nr), (1, nf)):
                for _ in range(cnt):
                    bs = bs + fk[w[strand]] * beta[q << 16 | n << 8 | k]
                    k += 1
                    w[strand] += 1
        return bs
    finally:
        L.orc_errmod_destroy(em)


@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_table_value_of_a_single_base_cell(gpu_ctx_factory, n_smpl):
    """A single-base cell inside the table: the likelihood of every genotype without its base is float32 of the sequential
    double sum, computed here read by read from the oracle's fk and beta -- for a cell that is one table entry (5 + 7 reads of
    quality 25) and for one that goes on from the entry (plus 2 + 3 of quality 14).  The device keeps that float in a plane of
    its own which no entry point hands out, so it is compared through the oracle: the oracle's likelihoods are checked against
    the sum, and the device's PL, QS and site fields against the oracle's."""
    special = [lambda ref: [reads(ref, 25, 1, 5), reads(ref, 25, 0, 7)],
               lambda ref: [reads(ref, 25, 1, 5), reads(ref, 25, 0, 7), reads(ref, 14, 1, 2), reads(ref, 14, 0, 3)]]
    tile, where = tile_with(n_smpl, special, 808 + n_smpl)
    want, cr = check(gpu_ctx_factory, tile)
    assert_sums_show(cr, where)
    for c, groups, n in ((where[0], [(25, 5, 7)], 12), (where[1], [(25, 5, 7), (14, 2, 3)], 17)):
        ref = (c // n_smpl) % 4
        a = np.float32(walk_sum(groups, n))
        assert a > 0 and int(cr["n"][c]) == n
        p = cr["p"][c].reshape(5, 5)
        for j in range(5):
            assert p[j, j] == (np.float32(0) if j == ref else a)
