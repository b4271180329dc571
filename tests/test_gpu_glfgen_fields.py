"""glfgen_kernel's phase A at the edges of every field of the rd word, against the oracle: mapQ 0 / 59 / 60 / 255, baseQ
just below and at min_baseQ, RD_SKIP and RD_DEL, min_dist tails over 25, soft clips with SCR on, every nt16 code ('=' and N
included) and N references.  Phase A works on four reads a lane as byte planes, so the tiles also have segments that start
and end off a multiple of four, a read count that is not a multiple of four, and few samples (the global-atomic mode).
The indel pass (p->aux words: baseQ below min_baseQ, seqQ under baseQ, every base type) takes the same planes."""
import numpy as np
import pytest

from bcftools_amd import abi, synth, host
from tests.helpers import orc
from tests.test_gpu_parity import assert_mplp_equal

pytestmark = pytest.mark.gpu


def edge_tile(seed, n_sites, n_smpl, depth, min_baseQ, drop_last):
    tile = synth.numpy_tile(seed, n_sites, n_smpl, depth=depth, var_rate=0.3, ref_n_rate=0.1, mapq255_rate=0.02)
    rng = np.random.default_rng(seed + 1)
    rd = tile.rd.astype(np.int64)
    n = len(rd)
    bq = rd & 0xff
    bq = np.where(rng.random(n) < 0.3, rng.choice([0, min_baseQ - 1, min_baseQ, min_baseQ + 1, 59, 60, 63, 93], n), bq)
    mq = (rd >> 8) & 0xff
    mq = np.where(rng.random(n) < 0.4, rng.choice([0, 1, 19, 20, 58, 59, 60, 61, 254, 255], n), mq)
    nt = (rd >> 16) & 15
    nt = np.where(rng.random(n) < 0.1, rng.integers(0, 16, n), nt)
    flags = (rd >> 20) & 3                                   # strand, soft clip
    flags = np.where(rng.random(n) < 0.2, rng.integers(0, 4, n), flags)
    skip = rng.random(n)
    extra = np.where(skip < 0.03, abi.RD_SKIP, np.where(skip < 0.06, abi.RD_DEL, np.where(skip < 0.07, abi.RD_SKIP | abi.RD_DEL, 0)))
    tail = rd >> 24
    tail = np.where(rng.random(n) < 0.3, rng.choice([0, 1, 24, 25, 26, 99, 255], n), tail)
    rd = bq | mq << 8 | nt << 16 | flags << 20 | extra | tail << 24
    off = tile.plp_off.astype(np.int64)
    if drop_last:                                            # a read count off a multiple of four: the last cell loses reads
        k = (n % 4) + 1 if n % 4 != 3 else 2
        k = min(k, int(off[-1] - off[-2]))
        rd = rd[:n - k]
        off[-1] -= k
    return host.HostTile(n_smpl, tile.ref16, off.astype(np.uint32), rd.astype(np.uint32), tile.epos[:len(rd)].copy())


@pytest.mark.parametrize("n_sites,n_smpl,depth,seed,min_baseQ", [
    (24, 300, 30.0, 61, 13),            # LDS mode, several site segments per workgroup
    (6, 1000, 17.0, 62, 13),            # LDS mode, segments of odd lengths
    (150, 3, 9.0, 63, 13),              # few samples: the global-atomic mode
    (90, 1, 25.0, 64, 20),
    (40, 50, 30.0, 65, 0),              # min_baseQ 0: every base quality passes
])
@pytest.mark.parametrize("drop_last", [False, True])
def test_phase_a_field_edges(gpu_ctx_factory, n_sites, n_smpl, depth, seed, min_baseQ, drop_last):
    tile = edge_tile(seed, n_sites, n_smpl, depth, min_baseQ, drop_last)
    assert len(tile.rd) == int(tile.plp_off[-1])
    if drop_last:
        assert len(tile.rd) % 4 != 0
    fmt = abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD | abi.FMT_QS | abi.FMT_SCR | abi.INFO_SCR | abi.FMT_SP
    cfg = abi.default_cfg(n_smpl, max_sites=n_sites, max_reads=len(tile.rd), fmt_flag=fmt)
    cfg.min_baseQ = min_baseQ
    want = orc.mpileup(cfg, tile)
    got = gpu_ctx_factory(cfg).mpileup(tile)
    assert_mplp_equal(got, want)
    assert (want.site["mq0"] > 0).any() and (want.site["anno"] != 0).any()


@pytest.mark.parametrize("n_sites,n_smpl,depth,seed", [
    (8, 300, 30.0, 71),                 # LDS mode
    (60, 3, 12.0, 72),                  # few samples: the global-atomic mode
])
def test_phase_a_indel_aux_edges(gpu_ctx_factory, n_sites, n_smpl, depth, seed):
    """The indel pass: ref_base -1, base and quality from p->aux (baseQ | seqQ << 8 | base << 16).  baseQ below min_baseQ
    takes type 0 and the read's own base quality, seqQ caps q; RD_SKIP reads are not seen."""
    min_baseQ = 13
    t = edge_tile(seed, n_sites, n_smpl, depth, min_baseQ, drop_last=True)
    rng = np.random.default_rng(seed + 2)
    n = len(t.rd)
    rd = t.rd.astype(np.int64) & ~np.int64(abi.RD_DEL)      # (deletions are not an indel-pass filter: left out)
    bq = np.where(rng.random(n) < 0.4, rng.choice([0, min_baseQ - 1, min_baseQ, min_baseQ + 1, 40, 93], n), rng.integers(0, 94, n))
    sq = np.where(rng.random(n) < 0.4, rng.choice([0, 1, 12, 13, 20, 255], n), rng.integers(0, 256, n))
    ty = rng.integers(0, 5, n)
    aux = (bq | sq << 8 | ty << 16).astype(np.uint32)
    tile = host.HostTile(n_smpl, np.zeros(n_sites, dtype=np.int8), t.plp_off, rd.astype(np.uint32), t.epos, aux=aux, is_indel=1)
    fmt = abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD
    cfg = abi.default_cfg(n_smpl, max_sites=n_sites, max_reads=n, fmt_flag=fmt, min_baseQ=min_baseQ)
    want = orc.mpileup(cfg, tile)
    got = gpu_ctx_factory(cfg).mpileup(tile)
    assert_mplp_equal(got, want)
