"""bcfgpu_call_rewrite_vcf: the sample columns of call records of VCF text input, rewritten on the device from the input records' own
columns around the caller's GT / PL / GQ planes.  The bytes and all n_sites + 1 offsets are compared exactly with the twin of
tests/helpers/callvcftext.py (itself pinned against the reference's goldens in tests/test_call_rewrite_text.py).  The inputs are
those of tests/helpers/callvcftextgen.py: 40 records with nals cycling 1..5 and alleles dropped at the front, in the middle, at the
end, all but the first, or not at all, columns of very unequal lengths whose runs start at all 16 alignments; 1, 3, 64, 65 and 257
samples -- one lane, a partial wavefront, one wavefront, one past it, one past the 256-lane workgroup; a site past one round; columns
and texts past the 15 360 bytes of a stage, which their own lanes handle from or to global memory."""
import ctypes as C

import numpy as np
import pytest

from bcftools_amd import abi, engine
from bcftools_amd.lib import check
from tests.helpers import callvcf, callvcftext, vcfdec
from tests.helpers.callvcfgen import cases as field_cases
from tests.helpers.callvcftextgen import N, STAGE, cases, one_site, past_one_round, past_the_stage, short_col
from tests.test_gpu_call_key_encode import check_equal, context
from tests.test_gpu_call_vcf_encode import Planes, mapped

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 64, 65, 257]


def run(ctx, case, S_in, col=None, emit=None, cap_bytes=None, gq=True):
    text, rec, site, planes, ngmax = case
    P = Planes(ctx, site, planes, gq=gq)
    return ctx.rewrite_call_vcf(P.out, len(site), ngmax, rec, S_in, text, col=col, emit=emit, cap_bytes=cap_bytes)


def twin_of(case, S_in, col=None, emit=None):
    text, rec, site, planes, ngmax = case
    if col is not None:                                             # the planes are the called samples': the map's many
        planes = {n: np.ascontiguousarray(a[..., :len(col)]) for n, a in planes.items()}
    return callvcftext.rewrite(planes, ngmax, rec, text, S_in, site, S_in if col is None else len(col), col, emit)


@pytest.fixture(scope="module")
def twin():
    """The twin's answer for a generated case, computed once."""
    memo = {}

    def get(S_in, col=None, emit=None):
        k = (S_in, None if col is None else tuple(col), None if emit is None else tuple(emit))
        if k not in memo:
            memo[k] = twin_of(cases(S_in), S_in, col, emit)
        return memo[k]
    return get


@pytest.mark.parametrize("S", SIZES)
def test_every_record_at_every_sample_count(S, twin):
    case = cases(S)
    assert {int(r["off"]) % 16 for r in case[1]} == set(range(16))
    with context(S) as ctx:
        got = run(ctx, case, S)
    exp = twin(S)
    check_equal(got, exp)
    sizes = np.diff(exp[1].astype(np.int64))
    assert (sizes > 0).all() and len({int(x) % 16 for x in exp[1][:-1]}) > 10          # the texts start at many alignments
    if S >= 65:
        assert sizes.max() > STAGE and int(case[1]["len"].max()) > STAGE               # more than one round, on both sides


def test_a_site_past_one_round():
    S = 65
    case = past_one_round(S)
    exp = twin_of(case, S)
    assert int(case[1]["len"][0]) > STAGE and len(exp[0]) > STAGE
    with context(S, 1) as ctx:
        check_equal(run(ctx, case, S), exp)
        check_equal(run(ctx, mapped(case, S), S, col=list(range(S))[::-1]), twin_of(case, S, list(range(S))[::-1]))


@pytest.mark.parametrize("which", ["both", "output", "input"])
@pytest.mark.parametrize("S", [1, 3])
def test_a_column_past_the_stage(which, S):
    """The slow paths: a column its lane reads from global memory, a text its lane writes there byte by byte -- alone and between
    short columns, without a map and with one (where every column is read in place)."""
    case = past_the_stage(which, S)
    exp = twin_of(case, S)
    col = list(range(S))[::-1]
    with context(S, 1) as ctx:
        check_equal(run(ctx, case, S), exp)
        check_equal(run(ctx, case, S, col=col), twin_of(case, S, col))
    longest = max(len(t) for t in exp[0].tobytes().split(b"\t"))
    assert (longest + 1 > STAGE) == (which != "input")


@pytest.mark.parametrize("S_in,which", [(65, "reversed"), (65, "three"), (65, "twice"), (257, "reversed"), (257, "three")])
def test_a_sample_map(S_in, which, twin):
    col = {"reversed": list(range(S_in))[::-1], "three": [41, 3, S_in - 1], "twice": [7, 64, 7, 0, 33]}[which]
    with context(len(col)) as ctx:
        got = run(ctx, mapped(cases(S_in), len(col)), S_in, col=col)
    check_equal(got, twin(S_in, col))


def test_an_identity_map_gives_the_same_bytes(twin):
    S = 65
    with context(S) as ctx:
        got = run(ctx, cases(S), S, col=list(range(S)))
    check_equal(got, twin(S))


def test_fewer_called_samples_without_a_map(twin):
    S_in, S = 65, 3
    with context(S) as ctx:
        got = run(ctx, mapped(cases(S_in), S), S_in)
    check_equal(got, twin(S_in, list(range(S))))


def test_emit_masks_and_no_sites(twin):
    S = 65
    case = cases(S)
    first, last = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    first[0], last[-1] = 1, 1
    with context(S) as ctx:
        for emit in (None, np.zeros(N, np.uint8), np.ones(N, np.uint8), (np.arange(N) % 3 != 1).astype(np.uint8), first, last):
            check_equal(run(ctx, case, S, emit=emit), twin(S, None, emit))
        P = Planes(ctx, case[2], case[3])
        data, off = ctx.rewrite_call_vcf(P.out, 0, case[4], case[1][:0], S, case[0])
        assert len(data) == 0 and off.tolist() == [0]
    assert len(twin(S, None, np.zeros(N, np.uint8))[0]) == 0


def raw_call(ctx, planes, n_sites, ngmax, rec, S_in, d_text, n_text, col, d_emit, d_buf, cap, d_off, nb):
    r = None if rec is None else np.ascontiguousarray(rec, dtype=abi.VCF_REWRITE)
    c = None if col is None else np.ascontiguousarray(col, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    return ctx.L.bcfgpu_call_rewrite_vcf(ctx.h, n_sites, ngmax, None if planes is None else C.byref(planes),
                                         None if r is None else r.ctypes.data_as(C.POINTER(abi.VcfRewrite)), S_in, d_text, n_text, c, d_emit,
                                         d_buf, cap, d_off, None if nb is None else C.byref(nb))


def test_nothing_is_written_outside_the_emitted_sites_bytes(twin):
    """The buffer lies inside a larger one that holds a pattern beforehand, 61 bytes in (no alignment to lean on); with every third
    site left out the bytes are the twin's and both margins keep the pattern -- each site's text went to its own
    [d_off[k], d_off[k + 1]) and nowhere else."""
    S = 65
    text, rec, site, planes, ngmax = cases(S)
    emit = (np.arange(N) % 3 != 1).astype(np.uint8)
    wdata, woff = twin(S, None, emit)
    need, front, back = len(wdata), 61, 4096
    with context(S) as ctx:
        P, d_text, d_emit = Planes(ctx, site, planes), ctx.to_device(text), ctx.to_device(emit)
        buf, off, nb = ctx.buf(front + need + back), ctx.buf(8 * (N + 1)), C.c_uint64(0)
        check(ctx.L.bcfgpu_memset(ctx.h, buf.ptr, 0xA5, front + need + back))
        assert raw_call(ctx, P.out, N, ngmax, rec, S, d_text.ptr, text.nbytes, None, d_emit.ptr, buf.ptr + front, need, off.ptr, nb) == 0 and nb.value == need
        got = buf.download(np.zeros(front + need + back, np.uint8))
        assert got[front:front + need].tobytes() == wdata.tobytes() and (got[:front] == 0xA5).all() and (got[front + need:] == 0xA5).all()
        np.testing.assert_array_equal(off.download(np.zeros(N + 1, np.uint64)), woff)


def test_sizes_and_bad_arguments(twin):
    """The size-only call; cap_bytes one byte short (E_RANGE, *n_bytes the size, nothing written, the offsets set all the same); then
    every E_ARG / E_RANGE case, each with nothing written."""
    S = 65
    text, rec, site, planes, ngmax = case = cases(S)
    wdata, woff = twin(S)
    need = len(wdata)
    with context(S) as ctx:
        P, d_text = Planes(ctx, site, planes), ctx.to_device(text)
        buf, off = ctx.buf(need), ctx.buf(8 * (N + 1))
        nb = C.c_uint64(0)
        base = dict(planes=P.out, n_sites=N, ngmax=ngmax, rec=rec, S_in=S, d_text=d_text.ptr, n_text=text.nbytes, col=None, d_emit=None)

        def call(d_buf, cap, d_off=off.ptr, nbytes=nb, **kw):
            a = dict(base)
            a.update(kw)
            return raw_call(ctx, a["planes"], a["n_sites"], a["ngmax"], a["rec"], a["S_in"], a["d_text"], a["n_text"], a["col"], a["d_emit"],
                            d_buf, cap, d_off, nbytes)

        def untouched():
            return (buf.download(np.zeros(need, np.uint8)) == 0xA5).all()

        def offsets():
            return off.download(np.zeros(N + 1, np.uint64))
        check(ctx.L.bcfgpu_memset(ctx.h, buf.ptr, 0xA5, need))
        assert call(None, 0) == abi.E_RANGE and nb.value == need                        # cap_bytes = 0 asks for the size
        np.testing.assert_array_equal(offsets(), woff)
        check(ctx.L.bcfgpu_memset(ctx.h, off.ptr, 0, 8 * (N + 1)))
        assert call(buf.ptr, need - 1) == abi.E_RANGE and nb.value == need and untouched()
        np.testing.assert_array_equal(offsets(), woff)
        with pytest.raises(engine.BcfGpuError) as e:
            run(ctx, case, S, cap_bytes=need - 1)
        assert e.value.code == abi.E_RANGE and e.value.needed == need

        def bad(code, field=None, value=None, j=None, **kw):
            r = rec.copy()
            if field:
                r[field][j] = value
            nb.value = 12345
            rc = call(kw.pop("d_buf", buf.ptr), need, rec=kw.pop("rec", r), **kw)
            assert rc == code and nb.value == 0 and untouched(), (field, value, kw)
        with_pl = int(np.nonzero(rec["flags"] & 1)[0][0])
        no_pl = int(np.nonzero(rec["pl_idx"] < 0)[0][0])
        with_gq = int(np.nonzero(rec["flags"] & 2)[0][0])
        for j in (0, N - 1):
            bad(abi.E_ARG, "n_fmt", 0, j); bad(abi.E_ARG, "n_fmt", 65, j); bad(abi.E_ARG, "n_fmt", -1, j)
            bad(abi.E_ARG, "nals", 0, j); bad(abi.E_ARG, "nals", 6, j)
        bad(abi.E_ARG, "pl_idx", int(rec["n_fmt"][with_pl]), with_pl); bad(abi.E_ARG, "pl_idx", 64, with_pl)
        bad(abi.E_ARG, "pl_idx", -1, with_pl)                                           # PL listed without a place
        bad(abi.E_ARG, "flags", 1, no_pl)
        bad(abi.E_ARG, ngmax=0); bad(abi.E_ARG, ngmax=16)
        bad(abi.E_ARG, col=[0] * (S - 1) + [S]); bad(abi.E_ARG, col=[-1] + [0] * (S - 1))
        bad(abi.E_ARG, planes=None); bad(abi.E_ARG, d_off=None); bad(abi.E_ARG, d_buf=None); bad(abi.E_ARG, d_text=None); bad(abi.E_ARG, rec=None)
        bad(abi.E_ARG, S_in=0); bad(abi.E_ARG, S_in=S - 1)                               # more called samples than input samples
        for name in ("site", "gt", "pl", "gq"):                                         # a listed plane that is NULL
            Q = Planes(ctx, site, planes)
            setattr(Q.out, name, None)
            bad(abi.E_ARG, planes=Q.out)
        assert call(buf.ptr, need, nbytes=None) == abi.E_ARG and untouched()
        # the indexing pass: a run that starts a byte late (no tab in front, a tab too few); one that ends a column early; one that
        # takes in the tab of the bytes behind it -- at the first, a middle and the last site
        for j in (0, N // 2, N - 1):
            bad(abi.E_ARG, "off", int(rec["off"][j]) + 1, j)
            first_col = bytes(text[int(rec["off"][j]) + 1:]).index(b"\t") + 1
            r = rec.copy()
            r["off"][j] += first_col; r["len"][j] -= first_col                          # from the second tab on: a column too few
            bad(abi.E_ARG, rec=r)
        bad(abi.E_ARG, S_in=S + 1, col=list(range(S)))                                   # every run has a column too few
        bad(abi.E_RANGE, "off", text.nbytes, 3); bad(abi.E_RANGE, "off", 2 ** 63, 3); bad(abi.E_RANGE, "len", 2 ** 32 - 1, 3)
        bad(abi.E_RANGE, n_text=int(rec["off"].max()) + 1)                               # the last run passes the end
        # a site without a record is checked like the others
        emit = np.ones(N, np.uint8)
        emit[5] = 0
        d_emit = ctx.to_device(emit)
        bad(abi.E_ARG, "nals", 0, 5, d_emit=d_emit.ptr)
        # after all of them the call still gives the twin's bytes; without GQ listed the gq plane may be NULL
        assert call(buf.ptr, need) == 0 and nb.value == need
        assert buf.download(np.zeros(need, np.uint8)).tobytes() == wdata.tobytes()
        np.testing.assert_array_equal(offsets(), woff)
        r = rec.copy()
        r["flags"] &= ~2
        Q = Planes(ctx, site, planes, gq=False)
        assert call(buf.ptr, need, rec=r, planes=Q.out) == 0 and 0 < nb.value < need


def test_more_sites_than_the_offsets_workspace_takes_at_once():
    """257 columns a record are 258 offsets: the sites the workspace takes at once follow from BCFGPU_VCFDEC_START_BYTES, and three
    more than that are two chunks.  The sites are eight different records in turn (the twin rewrites those eight)."""
    S, kinds = 257, 8
    fits = abi.VCFDEC_START_BYTES // 4 // (S + 1)
    n = fits + 3
    assert (S + 1) * 4 * n > abi.VCFDEC_START_BYTES >= (S + 1) * 4 * fits
    rng = np.random.default_rng(31)
    ones = [one_site([short_col(rng) for _ in range(S)], seed=40 + i, keep=((0, 2), (0, 1, 2), (0,), (1, 2))[i % 4]) for i in range(kinds)]
    ones = [(t, r, st, dict(pls, pl=np.ascontiguousarray(pls["pl"][:, :3])), 3) for t, r, st, pls, _ in ones]     # three PL planes: small uploads
    want = [twin_of(c, S)[0].tobytes() for c in ones]
    text = np.concatenate([c[0] for c in ones])
    base = np.cumsum([0] + [len(c[0]) for c in ones])
    pick = (5 * np.arange(n)) % kinds
    rec = np.concatenate([c[1] for c in ones])
    rec["off"] += base[:-1].astype(np.uint64)
    rec, site = rec[pick], np.concatenate([c[2] for c in ones])[pick]
    planes = {name: np.ascontiguousarray(np.concatenate([c[3][name] for c in ones])[pick]) for name in ("gt", "pl", "gq")}
    with context(S, n) as ctx:
        P = Planes(ctx, site, planes)
        data, off = ctx.rewrite_call_vcf(P.out, n, 3, rec, S, text)
    data = data.tobytes()
    assert len(off) == n + 1 and int(off[-1]) == len(data) == sum(len(want[i]) for i in pick)
    for k in (0, 1, fits - 1, fits, fits + 1, n - 1):
        assert data[int(off[k]):int(off[k + 1])] == want[pick[k]], k
    assert data == b"".join(want[i] for i in pick)


def test_the_result_does_not_depend_on_the_calls_before(twin):
    """One context: bcfgpu_call_decode_vcf, then the rewrite, then bcfgpu_call_encode_vcf, and the rewrite again after a rewrite of
    another case -- each result that of a fresh context (the twins'): the entries' workspace slots are neighbours, the indexing kernel
    and the size pass are shared."""
    S = 65
    case, other = cases(S), cases(S, seed=1)
    fcase = field_cases(S)
    vec = [(int(r["off"]), int(r["len"]), int(r["pl_idx"])) for r in case[1]]
    with context(S) as ctx:
        planes_in = ctx.decode_vcf(case[0], vec, S, 3)
        a = run(ctx, case, S)
        P = Planes(ctx, fcase[2], fcase[3])
        enc = ctx.encode_call_vcf(P.out, len(fcase[2]), fcase[4], fcase[1], S, fcase[0])
        run(ctx, other, S, col=list(range(S))[::-1])
        b = run(ctx, case, S)
    with context(S) as ctx:
        np.testing.assert_array_equal(planes_in, ctx.decode_vcf(case[0], vec, S, 3))
    np.testing.assert_array_equal(planes_in, vcfdec.decode_text(bytes(case[0]), vec, S, 3))
    check_equal(a, twin(S))
    check_equal(b, twin(S))
    check_equal(enc, callvcf.encode_fields(fcase[3], fcase[4], fcase[1], fcase[0], S, fcase[2], S))


def test_abi_mirror_and_symbol():
    from bcftools_amd import lib
    assert C.sizeof(abi.VcfRewrite) == 32 and np.dtype(abi.VCF_REWRITE).itemsize == 32 and np.dtype(callvcftext.REC_DTYPE) == np.dtype(abi.VCF_REWRITE)
    assert [f[0] for f in abi.VcfRewrite._fields_] == ["off", "r_mask", "len", "pl_idx", "n_fmt", "nals", "flags"]
    assert [getattr(abi.VcfRewrite, f).offset for f in ("off", "r_mask", "len", "pl_idx", "n_fmt", "nals", "flags")] == [0, 8, 16, 20, 24, 26, 28]
    assert abi.VCF_REWRITE_MAX_KEYS == callvcftext.MAX_KEYS == 64
    assert hasattr(lib.load(), "bcfgpu_call_rewrite_vcf")
