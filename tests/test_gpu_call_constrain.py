"""bcfgpu_call_constrain: the PL and AD / QS planes of `call -C alleles` records in the alleles of their targets, made on the device
from the planes the decoders write.  The planes are compared exactly with the numpy twin of tests/helpers/calsplanes.py (itself pinned
against the record rewrite behind the reference's nine goldens in tests/test_call_constrain_planes.py).  The shapes are the smallest
that reach every branch: 42 sites cycling through the ways a record meets its target, original and target allele counts 1..5; 1, 3,
64, 65 and 257 samples -- one lane, a partial wavefront, a full one, one past it, one past the 256-lane workgroup; n_in and n_out at,
and one above, what the sites need; both modes."""
import ctypes as C

import numpy as np
import pytest

from bcftools_amd import abi, engine
from tests.helpers import calsplanes as CP

pytestmark = pytest.mark.gpu

MISSING, VEND = abi.INT32_MISSING, abi.INT32_VECTOR_END
N = 42
SIZES = [1, 3, 64, 65, 257]
KINDS = ("unchanged", "found", "reordered", "one_new", "two_new", "unseen0", "past")
G, R = abi.CALS_NUMBER_G, abi.CALS_NUMBER_R


def sites(n=N):
    """(descriptors, the original allele count of every site).  Site r: kind r % 7, original alleles 1 + (r // 7 + r) % 5; the
    last original allele is the unseen one where there are two or more."""
    d = np.zeros(n, dtype=abi.CALS_SITE)
    nori = np.zeros(n, np.int32)
    for r in range(n):
        kind, no = KINDS[r % 7], 1 + (r // 7 + r) % 5
        unseen = no - 1 if no > 1 else 0
        seen = list(range(1, no - 1)) if unseen else list(range(1, no))     # the ALTs that are real alleles
        if kind == "unchanged":
            amap, changed = list(range(no)), 0
        elif kind == "found":
            amap, changed = [0] + seen[::2] + ([unseen] if unseen else []), 1
        elif kind == "reordered":
            amap, changed = [0] + seen[::-1] + ([unseen] if unseen else []), 1
        elif kind == "one_new":
            amap, changed = [0] + seen[:2] + [unseen] + ([unseen] if unseen else []), 1
        elif kind == "two_new":
            amap, changed = [0] + seen[:1] + [unseen, unseen] + ([unseen] if unseen else []), 1
        elif kind == "unseen0":
            unseen = 0
            amap, changed = [0] + list(range(1, no))[:3] + [no - 1], 1     # a new allele on the last original one
        else:
            amap, changed = [0, 3 * no + 2] + seen[:2] + ([unseen] if unseen else []), 1      # an allele the input has no plane of
        amap = amap[:5]
        d["n_new"][r], d["unseen"][r], d["changed"][r] = len(amap), unseen, changed
        d["amap"][r, :len(amap)] = amap
        d["amap"][r, len(amap):] = -7                               # not read
        nori[r] = no
    return d, nori


def planes(S, mode, n_in, seed=0):
    """[N][n_in][S] input planes: a site's vector has a value per genotype (mode G) or allele (mode R) of its original alleles,
    `end of vector` behind.  Sample s is of class s % 8 (shifted by the site, so that a cohort of one sample meets them all):
    0 plain, 1 '.', 2 a value short, 3 `missing` wherever the unseen allele is not part (the first fallback), 4 the same and at
    (0, unseen) (the second and third), 5 `missing` but at (unseen, unseen) (the third), 6 `missing` everywhere, 7 the first value
    `end of vector`."""
    rng = np.random.default_rng(100 * seed + S + mode)
    d, nori = sites()
    p = np.full((N, n_in, S), VEND, np.int64)
    for r in range(N):
        no = int(nori[r])
        w = no * (no + 1) // 2 if mode == G else no
        u = no - 1
        has_u = [False] * w
        if mode == G:
            for i in range(no):
                for j in range(i + 1):
                    has_u[CP.gt(i, j)] = u in (i, j)
        else:
            has_u[u] = True
        v = rng.integers(0, 256, (w, S)).astype(np.int64)
        for s in range(S):
            cls = (s + r) % 8
            if cls == 1:
                v[0, s], v[1:, s] = MISSING, VEND
            elif cls == 2:
                v[w - 1:, s] = VEND
            elif cls in (3, 4):
                v[[g for g in range(w) if not has_u[g]], s] = MISSING
                if cls == 4 and mode == G and no > 1:
                    v[CP.gt(0, u), s] = MISSING
            elif cls == 5:
                v[:w - 1, s] = MISSING
            elif cls == 6:
                v[:, s] = MISSING
            elif cls == 7:
                v[:, s] = VEND
        p[r, :w] = v
    return p.astype(np.int32), d


def context(S):
    return engine.Context(abi.default_cfg(S, max_sites=N, max_reads=64))


def widths(mode):
    return (15, 15) if mode == G else (5, 5)


@pytest.fixture(scope="module")
def twin():
    """The twin's answer for a case, computed once."""
    memo = {}

    def get(S, mode, n_in, n_out, seed=0):
        k = (S, mode, n_in, n_out, seed)
        if k not in memo:
            p, d = planes(S, mode, n_in, seed)
            taken = [0, 0, 0]
            memo[k] = (CP.constrain(p, d.astype(CP.SITE_DTYPE), n_out, mode, taken), taken)
        return memo[k]
    return get


def test_the_sites_reach_every_case():
    d, nori = sites()
    assert set(nori) == {1, 2, 3, 4, 5} and set(d["n_new"]) == {1, 2, 3, 4, 5}
    assert (d["changed"] == 0).sum() == N // 7 and (d["unseen"][d["changed"] == 1] == 0).any()
    am = [list(d["amap"][r, :d["n_new"][r]]) for r in range(N)]
    assert any(a != sorted(a) for a in am)                          # a > b in gt()
    assert any(len(a) - len(set(a)) >= 2 for a in am)               # two new alleles and the unseen one on one original
    assert any(max(a) * (max(a) + 1) // 2 >= 16 for a in am)        # past n_in


@pytest.mark.parametrize("mode", [G, R])
@pytest.mark.parametrize("S", SIZES)
def test_every_site_at_every_sample_count(S, mode, twin):
    w_in, w_out = widths(mode)
    for n_in, n_out in ((w_in, w_out), (w_in + 1, w_out + 1), (w_in, w_out + 1)):
        p, d = planes(S, mode, n_in)
        with context(S) as ctx:
            got = ctx.constrain_planes(p, d, n_out, mode)
        exp, taken = twin(S, mode, n_in, n_out)
        np.testing.assert_array_equal(got, exp)
        if mode == G and S >= 64:
            assert min(taken) > 0, taken                            # each of the three fallbacks supplied a value
        assert (exp == MISSING).any() and (exp[:, 1:] == VEND).any() and (exp >= 0).any()


def raw_call(ctx, mode, d, n_in, d_in, n_out, d_out, n=None):
    d = np.ascontiguousarray(d, dtype=abi.CALS_SITE)
    return ctx.L.bcfgpu_call_constrain(ctx.h, mode, len(d) if n is None else n, d.ctypes.data_as(C.POINTER(abi.CalsSite)), n_in, d_in, n_out, d_out)


@pytest.mark.parametrize("mode", [G, R])
def test_bad_arguments_write_nothing(mode, twin):
    S = 65
    n_in, n_out = widths(mode)
    p, d = planes(S, mode, n_in)
    nbytes = N * n_out * S * 4
    with context(S) as ctx:
        d_in, d_out = ctx.to_device(p.reshape(-1)), ctx.buf(nbytes + 64)

        def untouched():
            return (d_out.download(np.zeros(nbytes + 64, np.uint8)) == 0xA5).all()
        assert ctx.L.bcfgpu_memset(ctx.h, d_out.ptr, 0xA5, nbytes + 64) == 0

        def bad(field=None, value=None, r=10, **kw):
            k = d.copy()
            if field == "amap":
                k["amap"][r, 1] = value
            elif field:
                k[field][r] = value
            a = dict(mode=mode, n_in=n_in, d_in=d_in.ptr, n_out=n_out, d_out=d_out.ptr)
            a.update(kw)
            assert raw_call(ctx, a["mode"], k, a["n_in"], a["d_in"], a["n_out"], a["d_out"]) == abi.E_ARG and untouched(), (field, value, kw)
        assert d["changed"][10] and d["n_new"][10] >= 2
        bad("n_new", 0); bad("n_new", 6); bad("n_new", -1)
        bad("amap", -1)
        bad(d_in=None); bad(d_out=None)
        bad(mode=2); bad(mode=-1)
        bad(n_in=0); bad(n_out=0)
        big = int(np.argmax(d["n_new"] * d["changed"]))
        need = int(d["n_new"][big]) * (int(d["n_new"][big]) + 1) // 2 if mode == G else int(d["n_new"][big])
        bad(n_out=need - 1)                                         # a changed site's vector does not fit
        bad(d_out=d_in.ptr); bad(d_out=d_in.ptr + 4 * S); bad(d_in=d_out.ptr + nbytes - 4)       # overlapping buffers
        assert ctx.L.bcfgpu_call_constrain(ctx.h, mode, N, None, n_in, d_in.ptr, n_out, d_out.ptr) == abi.E_ARG and untouched()
        assert ctx.L.bcfgpu_call_constrain(None, mode, N, d.ctypes.data_as(C.POINTER(abi.CalsSite)), n_in, d_in.ptr, n_out, d_out.ptr) == abi.E_ARG
        assert raw_call(ctx, mode, d, n_in, None, n_out, None, n=0) == 0 and untouched()          # no sites: a success
        k = d.copy()
        k["n_new"][0], k["amap"][0] = 5, 0                          # an unchanged site may be wider than n_out: it is copied, not gathered
        assert not k["changed"][0]
        assert raw_call(ctx, mode, k, n_in, d_in.ptr, n_out, d_out.ptr) == 0
        got = d_out.download(np.zeros(N * n_out * S, np.int32)).reshape(N, n_out, S)
        np.testing.assert_array_equal(got, twin(S, mode, n_in, n_out)[0])
        assert (d_out.download(np.zeros(nbytes + 64, np.uint8))[nbytes:] == 0xA5).all()             # nothing behind the planes


def test_two_calls_in_a_row_give_the_second_call_s_answer(twin):
    """One context: a call, a call of the other mode on other planes, the first call again; and a decoder call between them."""
    S = 65
    p, d = planes(S, G, 15)
    q, _ = planes(S, R, 6, seed=1)
    with context(S) as ctx:
        a = ctx.constrain_planes(p, d, 15, G)
        b = ctx.constrain_planes(q, d[::-1].copy(), 5, R)
        ctx.decode_bcf(np.zeros(S, np.uint8), [(0, 1, 1)], S, 3)
        c = ctx.constrain_planes(p, d, 15, G)
    np.testing.assert_array_equal(a, twin(S, G, 15, 15)[0])
    np.testing.assert_array_equal(c, a)
    np.testing.assert_array_equal(b, CP.constrain(q, d[::-1].astype(CP.SITE_DTYPE), 5, R))


def test_abi_mirror_and_symbol():
    from bcftools_amd import lib
    assert C.sizeof(abi.CalsSite) == 32 and np.dtype(abi.CALS_SITE).itemsize == 32 and np.dtype(abi.CALS_SITE) == CP.SITE_DTYPE
    assert [f[0] for f in abi.CalsSite._fields_] == ["n_new", "unseen", "changed", "amap"]
    assert abi.CalsSite.amap.offset == 12
    assert hasattr(lib.load(), "bcfgpu_call_constrain")
