"""cfg.capQ and cfg.errmod_theta off their defaults, device against oracle.  Every other test runs with capQ 60 and the default
errmod_theta, where a slip in either side's reading of the fields cannot show.

capQ (bam2bcf.c:196-202: mapQ 255 -> DEF_MAPQ, then min(mapQ, capQ), then q = clamp(min(q, mapQ), 4, 63)) reaches glfgen_kernel's
packed 16-bit minimum, the keys' qualities, the mapQ >= 59 side of the bias histograms and the I16 mapQ sums.  The values: 20 is
DEF_MAPQ, so 19 / 20 / 21 tell "255 -> 20, then cap" from the other order; 58 / 59 straddle the histograms' last bin; 1 and 4
meet the lower clamp of q; 63 is the largest bcfgpu_create takes; 0 means 60.

errmod_theta (errmod.c: the tables of errmod_init(1 - theta), CALL_DEFTHETA 0.83 when <= 0) builds fk, beta and lhet of a context
in csrc/api.hip and from them the prefix table of the errmod walk: every PL comes from them.

The tests marked gpu need the device; the others are the oracle's half -- that the values move the planes at all."""
import ctypes as C

import numpy as np
import pytest

from bcftools_amd import abi, synth, host
from tests.helpers import orc
from tests.test_gpu_parity import assert_mplp_equal
from tests.test_gpu_glfgen_prefix import tile_with, reads

gpu = pytest.mark.gpu

FMT = abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD | abi.FMT_QS | abi.FMT_SCR | abi.INFO_SCR | abi.FMT_SP
SAMPLES = [4, 64]                        # global histograms; histograms in LDS (n_smpl >= 37)
CAPQS = [1, 4, 19, 20, 21, 58, 59, 60, 63]
MAPQS = [0, 1, 19, 20, 21, 58, 59, 60, 61, 254, 255]
N_SITES = 24
DEEP = 17000                             # entries of the listed cell: past the largest LDS key window (csrc/kernels.h, 16384)
_cache = {}


def cap_tiles(n_smpl):
    """(SNP tile, indel tile) of 24 sites, cells of about 20 reads and never a multiple of four, so that cells start and end inside
    phase A's groups of four reads; mapQ from MAPQS, base qualities from under min_baseQ to 93, both strands, every fourth site a
    variant in half the samples.  Cell n_smpl + 1 of the SNP tile holds DEEP entries, about one in 300 of them a usable read: it
    is listed for the launch that gives a deep cell a workgroup of its own.  The indel tile has the aux words of the indel pass
    (base quality | sequence quality << 8 | type << 16)."""
    if ("cap", n_smpl) in _cache:
        return _cache["cap", n_smpl]
    rng = np.random.default_rng(900 + n_smpl)
    tiles = []
    for is_indel in (0, 1):
        depths = rng.poisson(20, N_SITES * n_smpl).astype(np.int64)
        depths += depths % 4 == 0
        deep = n_smpl + 1
        if not is_indel:
            depths[deep] = DEEP + 1
        while depths.sum() % 4 == 0 or depths[-1] % 4 == 0:      # the whole tile ends inside a group of four as well
            depths[-1] += 1
        R = int(depths.sum())
        cell = np.repeat(np.arange(N_SITES * n_smpl), depths)
        site, smpl = cell // n_smpl, cell % n_smpl
        ref = site % 4
        alt = (site % 4 == 3) & (smpl % 2 == 0) & (rng.random(R) < 0.5)
        base = np.where(alt, (ref + 1) % 4, np.where(rng.random(R) < 0.02, rng.integers(0, 4, R), ref))
        bq = rng.integers(8, 94, R)
        if not is_indel:
            bq = np.where(cell == deep, np.where(rng.random(R) < 0.003, rng.choice([14, 17, 20, 41], R), 5), bq)
        mq = rng.choice(MAPQS, R)
        rd = bq | mq << 8 | (1 << base) << 16 | rng.integers(0, 2, R) << 20 | rng.integers(0, 40, R) << 24
        aux = None
        if is_indel:
            abq = np.where(rng.random(R) < 0.3, rng.choice([0, 12, 13, 14, 40, 93], R), rng.integers(0, 94, R))
            asq = np.where(rng.random(R) < 0.4, rng.choice([0, 1, 12, 13, 20, 255], R), rng.integers(0, 256, R))
            ty = np.where((site % 4 != 0) & (rng.random(R) < 0.3), rng.integers(1, 4, R), 0)
            aux = (abq | asq << 8 | ty << 16).astype(np.uint32)
        ref16 = np.zeros(N_SITES, np.int8) if is_indel else (1 << (np.arange(N_SITES) % 4)).astype(np.int8)
        t = host.HostTile(n_smpl, ref16, np.r_[0, np.cumsum(depths)].astype(np.uint32), rd.astype(np.uint32),
                          rng.integers(0, 100, R).astype(np.uint8), aux=aux, is_indel=is_indel)
        assert (np.diff(t.plp_off.astype(np.int64)) % 4 != 0).all()
        tiles.append(t)
    _cache["cap", n_smpl] = tiles
    return tiles


def cap_cfg(n_smpl, capQ, min_baseQ=13):
    snp, indel = cap_tiles(n_smpl)
    cfg = abi.default_cfg(n_smpl, max_sites=N_SITES, max_reads=max(len(snp.rd), len(indel.rd)), fmt_flag=FMT, min_baseQ=min_baseQ)
    cfg.capQ = capQ
    return cfg


def oracle_cap(n_smpl, capQ, min_baseQ=13):
    """The oracle's planes of both tiles, computed once per case and not changed afterwards."""
    key = ("capres", n_smpl, capQ, min_baseQ)
    if key not in _cache:
        _cache[key] = [orc.mpileup(cap_cfg(n_smpl, capQ, min_baseQ), t) for t in cap_tiles(n_smpl)]
    return _cache[key]


def planes_differ(a, b):
    return not np.array_equal(a.pl, b.pl) or not np.array_equal(a.site["anno"], b.site["anno"])


def assert_same_bytes(a, b):
    assert a.site.tobytes() == b.site.tobytes()
    for k in ["pl", "dp4", "adf", "adr", "qs", "scr", "sp"]:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)


@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_oracle_planes_move_with_capq(n_smpl):
    """Every capQ other than 60 gives other PL or I16 planes than 60 does, on the SNP tile and on the indel tile; and the tile has
    what the cases are about: usable reads of every mapQ, the deep cell with a few dozen of them."""
    snp, indel = cap_tiles(n_smpl)
    assert len(snp.rd) % 4 != 0 and len(indel.rd) % 4 != 0
    usable = (snp.rd & 0xff) >= 13
    assert set((snp.rd[usable] >> 8 & 0xff).tolist()) == set(MAPQS)
    a, b = int(snp.plp_off[n_smpl + 1]), int(snp.plp_off[n_smpl + 2])
    assert b - a > DEEP and 20 <= int(usable[a:b].sum()) < 255
    base = oracle_cap(n_smpl, 60)
    for capQ in CAPQS:
        if capQ != 60:
            got = oracle_cap(n_smpl, capQ)
            assert planes_differ(got[0], base[0]) and planes_differ(got[1], base[1]), capQ
    for r in base:
        assert (r.site["ret"] == 0).sum() >= 6 and (r.site["n_alleles"] > 2).any()
    assert_same_bytes(oracle_cap(n_smpl, 0)[0], base[0])


@gpu
@pytest.mark.parametrize("capQ", CAPQS)
@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_capq_matches_oracle(gpu_ctx_factory, n_smpl, capQ):
    ctx = gpu_ctx_factory(cap_cfg(n_smpl, capQ))
    for tile, want in zip(cap_tiles(n_smpl), oracle_cap(n_smpl, capQ)):
        assert_mplp_equal(ctx.mpileup(tile), want)


@gpu
@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_capq_zero_is_sixty(gpu_ctx_factory, n_smpl):
    c0, c60 = gpu_ctx_factory(cap_cfg(n_smpl, 0)), gpu_ctx_factory(cap_cfg(n_smpl, 60))
    for tile, want in zip(cap_tiles(n_smpl), oracle_cap(n_smpl, 60)):
        got = c0.mpileup(tile)
        assert_same_bytes(got, c60.mpileup(tile))
        assert_mplp_equal(got, want)


@gpu
def test_create_refuses_capq_past_63_and_takes_a_negative_min_baseq_as_zero(gpu_ctx_factory):
    from bcftools_amd import lib
    L = lib.load()
    cfg, h = cap_cfg(4, 64), C.c_void_p()
    assert L.bcfgpu_create(C.byref(cfg), C.byref(h)) == abi.E_ARG and not h.value
    assert b"capQ" in L.bcfgpu_last_error()
    # min_baseQ below 0: every base quality passes, as with 0
    want = oracle_cap(4, 60, min_baseQ=0)
    assert planes_differ(want[0], oracle_cap(4, 60)[0])
    neg, zero = gpu_ctx_factory(cap_cfg(4, 60, min_baseQ=-5)), gpu_ctx_factory(cap_cfg(4, 60, min_baseQ=0))
    for tile, w in zip(cap_tiles(4), want):
        got = neg.mpileup(tile)
        assert_same_bytes(got, zero.mpileup(tile))
        assert_mplp_equal(got, w)


# ---- errmod_theta ----

THETAS = [0.5, 0.83, 0.97]


def theta_tiles(n_smpl):
    """The crafted cells around the domain of the prefix table (tests/test_gpu_glfgen_prefix.py: looked up when n < 64 and the top
    quality has fewer than 32 reads on either strand, walked otherwise) among ordinary cells, and an ordinary tile at depth 30."""
    if ("theta", n_smpl) in _cache:
        return _cache["theta", n_smpl]
    low = lambda ref, k: [reads(ref, 14, 1, k // 2), reads(ref, 14, 0, k - k // 2)]
    special = []
    for k in (31, 32):
        special += [lambda ref, k=k: [reads(ref, 20, 1, k)] + low(ref, 5),
                    lambda ref, k=k: [reads(ref, 20, 0, k)] + low(ref, 5),
                    lambda ref, k=k: [reads(ref, 20, 1, k), reads(ref, 20, 0, 3)] + low(ref, 4),
                    lambda ref, k=k: [reads(ref, 20, 1, k), reads(ref, 20, 0, k)]]
    for n in (62, 63, 64, 65):
        special += [lambda ref, n=n: [reads(ref, 41, 1, 1)] + low(ref, n - 1),
                    lambda ref, n=n: [reads(ref, 41, 1, 1)] + low(ref, n - 4) + [reads((ref + 1) % 4, 14, 0, 3)]]
    special += [lambda ref: [reads(ref, 25, 1, 5), reads(ref, 25, 0, 7)],                      # one table entry, nothing to walk
                lambda ref: [reads(ref, 40, 1, 6), reads((ref + 1) % 4, 37, 0, 5), reads((ref + 1) % 4, 37, 1, 2)]]       # a het cell
    crafted, where = tile_with(n_smpl, special, 1200 + n_smpl)
    plain = synth.numpy_tile(1300 + n_smpl, N_SITES, n_smpl, depth=30.0, var_rate=0.25)
    _cache["theta", n_smpl] = [crafted, plain]
    return _cache["theta", n_smpl]


def theta_cfg(n_smpl, theta):
    tiles = theta_tiles(n_smpl)
    cfg = abi.default_cfg(n_smpl, max_sites=max(t.n_sites for t in tiles), max_reads=max(len(t.rd) for t in tiles),
                          fmt_flag=abi.INFO_VDB | abi.INFO_RPB | abi.FMT_AD | abi.FMT_QS | abi.FMT_SP)
    cfg.errmod_theta = theta
    return cfg


def oracle_theta(n_smpl, theta):
    key = ("thetares", n_smpl, theta)
    if key not in _cache:
        _cache[key] = [orc.mpileup(theta_cfg(n_smpl, theta), t) for t in theta_tiles(n_smpl)]
    return _cache[key]


@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_oracle_pl_moves_with_errmod_theta(n_smpl):
    base = oracle_theta(n_smpl, 0.83)
    for theta in (0.5, 0.97):
        for got, b in zip(oracle_theta(n_smpl, theta), base):
            assert not np.array_equal(got.pl, b.pl), theta
    for theta in (0.0, -1.0):
        for got, b in zip(oracle_theta(n_smpl, theta), base):
            assert_same_bytes(got, b)


@gpu
@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_errmod_theta_matches_oracle(gpu_ctx_factory, n_smpl, theta):
    ctx = gpu_ctx_factory(theta_cfg(n_smpl, theta))
    for tile, want in zip(theta_tiles(n_smpl), oracle_theta(n_smpl, theta)):
        assert_mplp_equal(ctx.mpileup(tile), want)


@gpu
@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_errmod_theta_unset_is_the_default(gpu_ctx_factory, n_smpl):
    dflt = gpu_ctx_factory(theta_cfg(n_smpl, 0.83))
    for theta in (0.0, -1.0):
        ctx = gpu_ctx_factory(theta_cfg(n_smpl, theta))
        for tile, want in zip(theta_tiles(n_smpl), oracle_theta(n_smpl, 0.83)):
            got = ctx.mpileup(tile)
            assert_same_bytes(got, dflt.mpileup(tile))
            assert_mplp_equal(got, want)


@gpu
@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_errmod_tables_belong_to_their_context(gpu_ctx_factory, n_smpl):
    """Two contexts of different errmod_theta alive at once and called in turn: each gives its own answer every time."""
    a, b = gpu_ctx_factory(theta_cfg(n_smpl, 0.5)), gpu_ctx_factory(theta_cfg(n_smpl, 0.97))
    wa, wb = oracle_theta(n_smpl, 0.5), oracle_theta(n_smpl, 0.97)
    for _ in range(2):
        for i, tile in enumerate(theta_tiles(n_smpl)):
            assert_mplp_equal(a.mpileup(tile), wa[i])
            assert_mplp_equal(b.mpileup(tile), wb[i])
    c = gpu_ctx_factory(theta_cfg(n_smpl, 0.83))               # a third, made after the others ran: theirs stay as they were
    assert_mplp_equal(c.mpileup(theta_tiles(n_smpl)[0]), oracle_theta(n_smpl, 0.83)[0])
    assert_mplp_equal(a.mpileup(theta_tiles(n_smpl)[0]), wa[0])
