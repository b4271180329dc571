"""glfgen_kernel's phase B where its key passes reach past a cell's slice, against the oracle.  The counting pass takes four
keys a trip whether or not they are the lane's own (up to three keys past the slice: the next cells' keys, or the slack behind
the key window), and pass 1 reads one key ahead.  So the tiles here put the end of a slice where what lies behind it differs:
the last cell of a workgroup empty, one to three reads deep, or ending with the tile's last read; a cell that ends with the
last key of a staging window (and the cells around that edge); lanes that go round again (more than ten qualities); het-heavy
tiles, where the counts of the other bases run; the indel pass; a cell worked on by the launch for listed cells (its keys in
the global scratch array).  Every case with the SCR fields off (mpileup's default: the soft-clip pass does not run) and on."""
import numpy as np
import pytest

from bcftools_amd import abi, synth, host
from tests.helpers import orc
from tests.test_gpu_parity import assert_mplp_equal, _lone_deep_cells

pytestmark = pytest.mark.gpu

WG = 256                                                        # cells per workgroup (csrc/glfgen.hip)
FMT = abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD | abi.FMT_QS | abi.FMT_SP
SCR = abi.FMT_SCR | abi.INFO_SCR


def trimmed(tile, depth_of, aux=None):
    """`tile` with the cells of `depth_of` (cell -> depth) cut to their first `depth` reads."""
    off = tile.plp_off.astype(np.int64)
    n = np.diff(off)
    keep = np.ones(len(tile.rd), bool)
    for c, d in depth_of.items():
        assert n[c] >= d, "cell %d has %d reads, %d wanted" % (c, n[c], d)
        keep[off[c] + d:off[c + 1]] = False
        n[c] = d
    new_off = np.r_[0, np.cumsum(n)].astype(np.uint32)
    if aux is None:
        return host.HostTile(tile.n_smpl, tile.ref16, new_off, tile.rd[keep].copy(), tile.epos[keep].copy())
    return host.HostTile(tile.n_smpl, tile.ref16, new_off, tile.rd[keep].copy(), tile.epos[keep].copy(), aux=aux[keep].copy(), is_indel=1)


def last_cells(n_cells):
    """The last cell of every workgroup (the tile's last cell among them)."""
    return sorted(set(list(range(WG - 1, n_cells, WG)) + [n_cells - 1]))


def check(gpu_ctx_factory, tile, n_sites, scr, **cfg_kw):
    cfg = abi.default_cfg(tile.n_smpl, max_sites=n_sites, max_reads=max(len(tile.rd), 1), fmt_flag=FMT | (SCR if scr else 0), **cfg_kw)
    want = orc.mpileup(cfg, tile)
    got = gpu_ctx_factory(cfg).mpileup(tile)
    assert_mplp_equal(got, want)
    return want


@pytest.mark.parametrize("scr", [False, True])
@pytest.mark.parametrize("last_depth", [0, 1, 2, 3, None])
@pytest.mark.parametrize("n_sites,n_smpl,depth,var_rate,wide_qual,seed", [
    (3, 300, 30.0, 0.01, False, 81),        # 900 cells: workgroups end inside a site, the last one is short
    (4, 128, 30.0, 0.3, False, 82),         # het-heavy: the counts of the other bases run; the tile ends with a full workgroup
    (3, 300, 40.0, 0.3, True, 83),          # unbinned qualities: more than ten a cell, every lane goes round again
    (70, 5, 12.0, 0.3, True, 84),           # few samples: the global-histogram mode
])
def test_last_cell_of_a_workgroup(gpu_ctx_factory, n_sites, n_smpl, depth, var_rate, wide_qual, seed, last_depth, scr):
    """The keys behind the slice of a workgroup's last cell are nobody's (stale keys of an earlier round, or the slack): the cell
    empty, one to three reads deep (less than a trip of the count), or as drawn (None; the tile's last cell then ends with the
    tile's last read, as it does in every case)."""
    tile = synth.numpy_tile(seed, n_sites, n_smpl, depth=depth, var_rate=var_rate, wide_qual=wide_qual)
    if last_depth is not None:
        tile = trimmed(tile, {c: last_depth for c in last_cells(n_sites * n_smpl)})
        n = np.diff(tile.plp_off.astype(np.int64))
        assert all(n[c] == last_depth for c in last_cells(n_sites * n_smpl))
    assert len(tile.rd) == int(tile.plp_off[-1])
    if wide_qual:                                               # a second round: more than ten qualities among a cell's reads
        off = tile.plp_off.astype(np.int64)
        q = np.clip(np.minimum(tile.rd & 0xff, (tile.rd >> 8) & 0xff), 4, 63)
        usable = (tile.rd & 0xff) >= 13
        assert max(len(np.unique(q[off[c]:off[c + 1]][usable[off[c]:off[c + 1]]])) for c in range(0, n_sites * n_smpl, 7)) > 10
    want = check(gpu_ctx_factory, tile, n_sites, scr)
    if scr:
        assert (want.scr != 0).any()


@pytest.mark.parametrize("scr", [False, True])
def test_cell_that_ends_with_the_staging_window(gpu_ctx_factory, scr):
    """A workgroup whose span does not fit its key window works it off in rounds.  One hundred cells of 60 reads, then a cell
    whose last read is swept over the window's last key (6016 keys for a shallow tile of 300 samples, csrc/api.hip; the sweep
    covers any window between 5984 and 6040): the cell that ends exactly there reads the slack behind the window, the ones
    that end past it open the next round.  Cells of one to three reads follow."""
    n_smpl = 300
    base = synth.numpy_tile(91, 1, n_smpl, depth=90.0, var_rate=0.3)
    n = np.diff(base.plp_off.astype(np.int64))
    assert (n[:101] >= 60).all()
    ctx = None
    for d in range(0, 57):
        depth_of = {c: 60 for c in range(100)}
        depth_of[100] = d                                       # the span reaches 5984 + d keys with this cell
        depth_of.update({c: 1 + c % 3 for c in range(101, n_smpl)})
        tile = trimmed(base, depth_of)
        cfg = abi.default_cfg(n_smpl, max_sites=1, max_reads=8000, fmt_flag=FMT | (SCR if scr else 0))
        ctx = ctx or gpu_ctx_factory(cfg)
        assert_mplp_equal(ctx.mpileup(tile), orc.mpileup(cfg, tile))


@pytest.mark.parametrize("scr", [False, True])
@pytest.mark.parametrize("last_depth", [0, 2, None])
def test_indel_pass_last_cells(gpu_ctx_factory, last_depth, scr):
    """The indel pass (quality and type from p->aux, every cell's primary type 0) on the same tile ends."""
    n_sites, n_smpl, seed = 3, 300, 95
    t = synth.numpy_tile(seed, n_sites, n_smpl, depth=25.0, var_rate=0.0)
    rng = np.random.default_rng(seed + 2)
    n = len(t.rd)
    bq = rng.choice([5, 13, 20, 30, 40, 60], n)
    sq = rng.choice([12, 20, 40, 255], n)
    ty = np.where(rng.random(n) < 0.3, rng.integers(1, 5, n), 0)
    aux = (bq | sq << 8 | ty << 16).astype(np.uint32)
    tile = trimmed(t, {} if last_depth is None else {c: last_depth for c in last_cells(n_sites * n_smpl)}, aux=aux)
    tile = host.HostTile(n_smpl, np.zeros(n_sites, dtype=np.int8), tile.plp_off, tile.rd, tile.epos, aux=tile.aux, is_indel=1)
    check(gpu_ctx_factory, tile, n_sites, scr, min_baseQ=13)


@pytest.mark.parametrize("scr", [False, True])
@pytest.mark.parametrize("where", [[5], [119]])
def test_listed_cell(gpu_ctx_factory, where, scr):
    """A cell deeper than any key window goes to the launch for listed cells: its keys lie in the global scratch array, with the
    slack that launch leaves behind them; as the tile's last cell it ends with the tile's last read."""
    n_smpl, n_sites, seed = 40, 3, 97
    rng = np.random.default_rng(seed)
    depths = rng.poisson(12, n_sites * n_smpl).astype(np.int64)
    depths[where[0]] = 7001
    tile = _lone_deep_cells(n_smpl, depths, seed, usable_frac=0.02, n_sites=n_sites)
    off = tile.plp_off.astype(np.int64)
    cell = np.repeat(np.arange(n_sites * n_smpl), np.diff(off))
    plain = ~np.isin(cell, where)
    tile.rd[plain] = (tile.rd[plain] & ~np.uint32(0xff)) | rng.choice([11, 25, 37, 40], int(plain.sum())).astype(np.uint32)
    tile.rd[:] = tile.rd | (rng.random(len(tile.rd)) < 0.1).astype(np.uint32) << 21          # soft clips
    check(gpu_ctx_factory, tile, n_sites, scr)
