"""bcfgpu_pileup / bcfgpu_pileup_packed / bcfgpu_pileup_entries on directed pools (tests/helpers/cigargen.py) against
cigargen.expanded_pileup, a reference of another shape than the kernel's walk: every CIGAR class, reads up to the fields' limits
and the refusal past them, a candidate window far wider than the reads, ties, tile shapes at the work mapping's edges, the LDS
staging's capacity and the byte copy's alignments.  Every comparison is exact.  What each pool reaches, and that it tells a changed
rule from the rule, is asserted on the CPU in tests/test_pileup_twins.py."""
import numpy as np
import pytest

from bcftools_amd import abi
from bcftools_amd.lib import check, BcfGpuError
from tests.helpers import cigargen as G
from tests.test_gpu_pileup import device_pileup, assert_tiles_equal

pytestmark = pytest.mark.gpu

_contexts = {}


def _context(factory, S, want_epos=True):
    """One context per sample count and fmt_flag for the module (a context's sample count is fixed)."""
    if (S, want_epos) not in _contexts:
        fmt = abi.INFO_VDB | abi.INFO_RPB if want_epos else abi.FMT_DP
        _contexts[S, want_epos] = factory(abi.default_cfg(S, max_sites=1, max_reads=64, fmt_flag=fmt))
    return _contexts[S, want_epos]


def _explain(case, region, got, want, entries):
    """The first entry that differs: sample, read, position, expected and actual word."""
    S, beg = want.n_smpl, case.regions[region][0]
    if not np.array_equal(got.plp_off, want.plp_off):
        cell = int(np.nonzero(got.plp_off != want.plp_off)[0][0]) - 1
        return "%s: cell (position %d, sample %d) holds %d entries, expected %d" % (
            case.name, beg + cell // S, cell % S, int(got.plp_off[cell + 1]) - int(got.plp_off[cell]), int(want.plp_off[cell + 1] - want.plp_off[cell]))
    bad = np.nonzero((got.rd != want.rd) | (got.epos != want.epos))[0]
    if len(bad) == 0:
        return ""
    i = int(bad[0])
    cell = int(np.searchsorted(want.plp_off, i, side="right")) - 1
    site = cell // S
    ri, qpos, indel = entries[site][i - int(want.plp_off[site * S])]
    r = case.pool[ri]
    return "%s: sample %d read %d (%s, pos %d) at position %d (qpos %d): word %#010x epos %d, expected %#010x epos %d" % (
        case.name, cell % S, ri, r.name, r.pos, beg + site, qpos, int(got.rd[i]), int(got.epos[i]), int(want.rd[i]), int(want.epos[i]))


def _run(factory, name, region=0, want_epos=True, packed=None):
    """The device's tile of a case's region against the reference; returns the context (with that pileup on it) and the reference."""
    case = G.cases()[name]
    want, w_n, w_indel, entries = ref = G.reference(name, region, want_epos)
    ctx = _context(factory, len(case.by_sample), want_epos)
    beg, end = case.regions[region]
    got, col_n, col_indel, _ = device_pileup(ctx, case.by_sample, case.refseq, beg, end, packed=packed)
    why = _explain(case, region, got, want, entries)
    if why:
        print(why)
    assert_tiles_equal(got, want)
    np.testing.assert_array_equal(col_n, w_n)
    np.testing.assert_array_equal(col_indel, w_indel)
    return ctx, ref


# ---- 1. CIGAR classes ----
@pytest.mark.parametrize("packed", [None, "seq+qual+off"])
@pytest.mark.parametrize("want_epos", [True, False])
def test_cigar_classes(gpu_ctx_factory, want_epos, packed):
    _, (want, _, w_indel, _) = _run(gpu_ctx_factory, "classes", 0, want_epos, packed)
    assert w_indel.any() and want.epos.any() == want_epos


# ---- 2. entries ----
def _assert_entries(ctx, ref, cols):
    """bcfgpu_pileup_entries of columns `cols` of the pileup on ctx against the reference's; returns (read, qpos, indel)."""
    want, w_n, _, entries = ref
    S = want.n_smpl
    cap = int(w_n[cols].sum())
    so = np.zeros(len(cols) * S + 1, np.int32)
    pr, pq, pi = (np.zeros(cap, np.int32) for _ in range(3))
    check(ctx.L.bcfgpu_pileup_entries(ctx.h, len(cols), cols.ctypes.data, so.ctypes.data, pr.ctypes.data, pq.ctypes.data,
                                       pi.ctypes.data, cap))
    off = want.plp_off.astype(np.int64)
    cells = (cols[:, None].astype(np.int64) * S + np.arange(S)[None, :]).ravel()
    np.testing.assert_array_equal(so, np.concatenate([[0], np.cumsum(off[cells + 1] - off[cells])]).astype(np.int32))
    flat = [t for c in cols for t in entries[int(c)]]
    for k, (got, name) in enumerate(((pr, "read"), (pq, "qpos"), (pi, "indel"))):
        np.testing.assert_array_equal(got, np.array([t[k] for t in flat], np.int32), err_msg=name)
    return pr, pq, pi


def test_entries_of_the_classes(gpu_ctx_factory):
    """bcfgpu_pileup_entries (resolve_cigar, the fill pass's walk, from a wavefront per cell): every column with an indel and ten without."""
    ctx, ref = _run(gpu_ctx_factory, "classes")
    _, w_n, w_indel, _ = ref
    plain = np.nonzero((w_indel == 0) & (w_n > 0))[0]
    cols = np.sort(np.concatenate([np.nonzero(w_indel)[0], plain[:: max(1, len(plain) // 10)][:10]])).astype(np.int32)
    assert (w_indel[cols] == 0).sum() == 10 and w_indel[cols].sum() == w_indel.sum() > 5
    _, _, pi = _assert_entries(ctx, ref, cols)
    assert {2, 3, 4, -1, -2} <= set(pi.tolist())


@pytest.mark.parametrize("name", ["classes", "shape_17x17", "shape_33x16"])
def test_entries_of_every_column(gpu_ctx_factory, name):
    """The entries' query offset and indel in every column that has entries -- one entry per record of the tile, in the tile's
    order -- so that the columns inside a deletion and inside a reference skip, those of soft-clipped reads, the last base before
    pads and an insertion, before consecutive insertions and before a deletion are all among them; two tiles of fewer than 64
    columns that cross the 16-column edge of the fill pass's workgroups beside the classes."""
    ctx, ref = _run(gpu_ctx_factory, name)
    want, w_n, _, _ = ref
    pr, pq, pi = _assert_entries(ctx, ref, np.nonzero(w_n > 0)[0].astype(np.int32))
    assert len(pr) == len(want.rd) > 0
    if name == "classes":
        pool = G.cases()[name].pool
        for flag in (abi.RD_DEL, abi.RD_SKIP, abi.RD_SCLIP):
            assert (want.rd & flag).any()
        assert ((want.rd & abi.RD_SCLIP) != 0)[pq > 0].any()                   # a soft clip before the entry's base
        by_class = {}
        for r, d in zip(pr.tolist(), pi.tolist()):
            by_class.setdefault(pool[r].name, set()).add(d)
        assert 3 in by_class["M_P_I_P_I_M"] and 4 in by_class["M_I_I_M"] and -2 in by_class["M_P_D_M"] and -2 in by_class["M_D"]
        assert by_class["M_N_M"] == {0} and by_class["M_N"] == {0}


# ---- 3. window and ties ----
def test_window_far_wider_than_the_reads_and_ties(gpu_ctx_factory):
    """max_span = 20 060 from one read: the candidate window of every column holds all the short reads before it; in the middle
    of the skip the long read is every cell's first entry, as a deletion and a reference skip."""
    for region in range(4):
        _, (want, w_n, _, entries) = _run(gpu_ctx_factory, "window", region)
        if region == 1:
            first = want.rd[want.plp_off[:-1:3]]
            assert ((first & (abi.RD_DEL | abi.RD_SKIP)) == (abi.RD_DEL | abi.RD_SKIP)).all() and all(col[0][0] == 0 for col in entries)
            assert w_n.max() >= 40                                          # the 40 reads at one position


# ---- 4. long reads and the field limits ----
def test_long_reads(gpu_ctx_factory):
    """Reads of 255 ... 65 535 bases (lq and ntot at the last value of their 16 bits, the tail distance past its clamp), ~200
    operations, a 20 000-base skip."""
    tails = set()
    for region in range(len(G.cases()["long"].regions)):
        _, (want, _, _, _) = _run(gpu_ctx_factory, "long", region)
        tails.update((want.rd >> 24).tolist())
    assert {0, 253, 254, 255} <= tails


def test_reads_past_the_field_limits_are_refused_and_the_context_goes_on(gpu_ctx_factory):
    ctx = _context(gpu_ctx_factory, 3)
    for bad in (G.too_long_read(), G.too_many_ops_read()):
        with pytest.raises(BcfGpuError) as e:
            device_pileup(ctx, [[bad], [], []], "ACGT" * 20, 20, 60)
        assert e.value.code == abi.E_RANGE
        assert _run(gpu_ctx_factory, "classes")[0] is ctx                  # 255 operations are accepted (class M1I1_255ops)
    ok = next(r for r in G.cases()["long"].pool if r.l_qseq == 65535)       # and 65 535 bases
    got, _, _, _ = device_pileup(ctx, [[], [ok], []], "ACGT" * 20, ok.end - 8, ok.end + 8)
    want, _, _, _ = G.expanded_pileup([[], [ok], []], "ACGT" * 20, ok.end - 8, ok.end + 8)
    assert_tiles_equal(got, want)
    assert len(want.rd) == 8


# ---- 5. tile shapes ----
@pytest.mark.parametrize("n_sites,S", G.SHAPES)
def test_tile_shapes(gpu_ctx_factory, n_sites, S):
    _, (want, w_n, _, _) = _run(gpu_ctx_factory, "shape_%dx%d" % (n_sites, S))
    assert len(want.rd) > 0
    if S > 1:                                                                # sample 1: no read at the first and the last column
        cells = np.array([1, (n_sites - 1) * S + 1])
        assert (want.plp_off[cells + 1] == want.plp_off[cells]).all()


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_pools_of_a_few_reads(gpu_ctx_factory, n):
    _, (want, w_n, _, entries) = _run(gpu_ctx_factory, "pool_of_%d" % n)
    assert w_n.max() == n and any(t[0] == n - 1 for col in entries for t in col)      # the pool's last read is in a column


def test_three_reads_in_order_at_one_position(gpu_ctx_factory):
    _run(gpu_ctx_factory, "three_in_order")


# ---- 6. staging boundary and the byte copy ----
@pytest.mark.parametrize("extra", [0, 1])
def test_staging_capacity(gpu_ctx_factory, extra):
    _, (want, _, _, _) = _run(gpu_ctx_factory, "staging_%d" % (9216 + extra))
    assert int(want.plp_off[16 * 16]) == 9216 + extra


def test_epos_copy_at_every_alignment(gpu_ctx_factory):
    _run(gpu_ctx_factory, "alignment")
