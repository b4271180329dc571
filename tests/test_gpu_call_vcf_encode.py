"""bcfgpu_call_encode_vcf: the sample columns of call records as VCF text, the caller's GT / PL / GQ planes and the pass-through keys
of the input records' bytes interleaved in FORMAT order, made on the device.  The bytes and all n_sites + 1 offsets are compared
exactly with the twin of tests/helpers/callvcf.py (itself pinned against the reference's goldens in
tests/test_call_sample_text.py).  The inputs are those of tests/helpers/callvcfgen.py: 37 records with nals cycling 1..5 and alleles
dropped at the front, in the middle, at the end, all but the first, or not at all; 1, 3, 64, 65 and 257 samples -- one lane, a
partial wavefront, one wavefront, one past it, one past the 256-lane workgroup; with the 255-value int32 key a sample's text passes
1 024 bytes and a site's block the 15 360 bytes of a round."""
import ctypes as C

import numpy as np
import pytest

from bcftools_amd import abi, engine
from bcftools_amd.lib import check
from tests.helpers import callvcf
from tests.helpers.callvcfgen import cases
from tests.test_gpu_call_key_encode import N, check_equal, context, jobs

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 64, 65, 257]


class Planes:
    """The call planes of a case in HBM: an abi.CallOut of device pointers (gp is not read)."""
    def __init__(self, ctx, site, planes, gq=True):
        self.bufs = {"site": ctx.to_device(site.view(np.uint8).reshape(-1)), "gt": ctx.to_device(planes["gt"]), "pl": ctx.to_device(planes["pl"])}
        if gq:
            self.bufs["gq"] = ctx.to_device(planes["gq"])
        self.out = abi.CallOut()
        for k, b in self.bufs.items():
            setattr(self.out, k, b.ptr)


def run(ctx, case, S_in, col=None, emit=None, cap_bytes=None):
    indiv, fields, site, planes, ngmax = case
    P = Planes(ctx, site, planes)
    return ctx.encode_call_vcf(P.out, len(site), ngmax, fields, S_in, indiv, col=col, emit=emit, cap_bytes=cap_bytes)


@pytest.fixture(scope="module")
def twin():
    """The twin's answer for a case, computed once."""
    memo = {}

    def get(S_in, col=None, emit=None):
        k = (S_in, None if col is None else tuple(col), None if emit is None else tuple(emit))
        if k not in memo:
            indiv, fields, site, planes, ngmax = cases(S_in)
            if col is not None:                                     # the planes are the called samples': the map's many
                planes = {n: np.ascontiguousarray(a[..., :len(col)]) for n, a in planes.items()}
            memo[k] = callvcf.encode_fields(planes, ngmax, fields, indiv, S_in, site, S_in if col is None else len(col), col, emit)
        return memo[k]
    return get


def mapped(case, n):
    """The case with call planes of n called samples (the first n columns of its planes)."""
    indiv, fields, site, planes, ngmax = case
    return indiv, fields, site, {k: np.ascontiguousarray(a[..., :n]) for k, a in planes.items()}, ngmax


@pytest.mark.parametrize("S", SIZES)
def test_every_field_at_every_sample_count(S, twin):
    case = cases(S)
    assert {int(f["off"]) % 16 for f in case[1] if f["kind"] == callvcf.KEY and f["type"] and f["width"]} == set(range(16))
    with context(S) as ctx:
        got = run(ctx, case, S)
    exp = twin(S)
    check_equal(got, exp)
    sizes = np.diff(exp[1].astype(np.int64))
    assert (sizes > 0).all() and len({int(x) % 16 for x in exp[1][:-1]}) > 10          # the blocks start at many alignments
    if S >= 65:
        assert sizes.max() > abi.VCF_SAMPLE_CAP                                         # more than one round
    text = exp[0].tobytes().split(b"\t")
    assert max(len(t) for t in text) > 1024                                             # a sample's text longer than 1 024 bytes


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
    """cfg.n_smpl below n_smpl_in and no map: called sample s is input sample s."""
    S_in, S = 65, 3
    with context(S) as ctx:
        got = run(ctx, mapped(cases(S_in), S), S_in)
    check_equal(got, twin(S_in, list(range(S))))


def test_emit_masks_and_no_fields(twin):
    S = 65
    case = cases(S)
    first, last = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    first[0], last[-1] = 1, 1
    with context(S) as ctx:
        for emit in (None, np.zeros(N, np.uint8), np.ones(N, np.uint8), (np.arange(N) % 3 != 1).astype(np.uint8), first, last):
            check_equal(run(ctx, case, S, emit=emit), twin(S, None, emit))
        data, off = run(ctx, (case[0], case[1][:0]) + case[2:], S)
        assert len(data) == 0 and off.tolist() == [0] * (N + 1)
        # a site in the middle without a field: zero length, its neighbours as they are
        f = case[1][case[1]["site"] != 7]
        check_equal(run(ctx, (case[0], f) + case[2:], S), callvcf.encode_fields(case[3], case[4], f, case[0], S, case[2], S))
        # no sites at all
        P = Planes(ctx, case[2], case[3])
        data, off = ctx.encode_call_vcf(P.out, 0, case[4], case[1][:0], S, case[0])
        assert len(data) == 0 and off.tolist() == [0]
    assert len(twin(S, None, np.zeros(N, np.uint8))[0]) == 0


def raw_call(ctx, planes, n_sites, ngmax, fields, S_in, d_indiv, n_indiv, col, d_emit, d_buf, cap, d_off, nb):
    f = np.ascontiguousarray(fields, dtype=abi.VCF_FIELD)
    c = None if col is None else np.ascontiguousarray(col, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    return ctx.L.bcfgpu_call_encode_vcf(ctx.h, n_sites, ngmax, None if planes is None else C.byref(planes), len(f), f.ctypes.data_as(C.POINTER(abi.VcfField)),
                                        S_in, d_indiv, n_indiv, c, d_emit, d_buf, cap, d_off, None if nb is None else C.byref(nb))


def test_sizes_and_bad_arguments(twin):
    """The size-only call; cap_bytes one byte short (E_RANGE, *n_bytes the size, nothing written, the offsets set all the same); then
    every E_ARG / E_RANGE case, each with nothing written."""
    S = 65
    indiv, fields, site, planes, ngmax = case = cases(S)
    wdata, woff = twin(S)
    need = len(wdata)
    with context(S) as ctx:
        P, d_in = Planes(ctx, site, planes), ctx.to_device(indiv)
        buf, off = ctx.buf(need), ctx.buf(8 * (N + 1))
        nb = C.c_uint64(0)
        base = dict(planes=P.out, n_sites=N, ngmax=ngmax, fields=fields, S_in=S, d_indiv=d_in.ptr, n_indiv=indiv.nbytes, col=None, d_emit=None)

        def call(d_buf, cap, d_off=off.ptr, nbytes=nb, **kw):
            a = dict(base)
            a.update(kw)
            return raw_call(ctx, a["planes"], a["n_sites"], a["ngmax"], a["fields"], a["S_in"], a["d_indiv"], a["n_indiv"], a["col"], a["d_emit"],
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
            f = fields.copy()
            if field:
                f[field][j] = value
            nb.value = 12345
            rc = call(kw.pop("d_buf", buf.ptr), need, fields=kw.pop("fields", f), **kw)
            assert rc == code and nb.value == 0 and untouched(), (field, value, kw)
        keys = np.nonzero(fields["kind"] == callvcf.KEY)[0]
        rkey = int(keys[0])                                                             # (the first key of a record is its R key)
        assert fields["flags"][rkey] & 1
        for k in (int(keys[4]), rkey):
            bad(abi.E_ARG, "type", 4, k); bad(abi.E_ARG, "type", -1, k); bad(abi.E_ARG, "width", -1, k); bad(abi.E_ARG, "width", 256, k)
        bad(abi.E_ARG, "site", -1, 0); bad(abi.E_ARG, "site", N, len(fields) - 1)
        bad(abi.E_ARG, "site", 0, len(fields) - 1)                                      # decreasing sites
        bad(abi.E_ARG, "site", 5, 0)
        bad(abi.E_ARG, "kind", 4, 3); bad(abi.E_ARG, "kind", -1, 3)
        bad(abi.E_ARG, "nals", 0, rkey); bad(abi.E_ARG, "nals", 6, rkey)
        bad(abi.E_ARG, col=[0] * (S - 1) + [S]); bad(abi.E_ARG, col=[-1] + [0] * (S - 1))
        bad(abi.E_ARG, planes=None); bad(abi.E_ARG, d_off=None); bad(abi.E_ARG, d_buf=None); bad(abi.E_ARG, d_indiv=None)
        bad(abi.E_ARG, S_in=0); bad(abi.E_ARG, S_in=S - 1)                               # more called samples than input samples
        bad(abi.E_ARG, ngmax=0); bad(abi.E_ARG, ngmax=16)
        for name in ("site", "gt", "pl", "gq"):                                         # a listed plane that is NULL
            Q = Planes(ctx, site, planes)
            setattr(Q.out, name, None)
            bad(abi.E_ARG, planes=Q.out)
        assert call(buf.ptr, need, nbytes=None) == abi.E_ARG and untouched()
        seventeen = np.zeros(17, dtype=abi.VCF_FIELD)                                   # 17 fields at one site
        seventeen["site"], seventeen["kind"] = 3, callvcf.GT
        bad(abi.E_ARG, fields=seventeen)
        assert call(buf.ptr, need, fields=seventeen[:16]) == 0 and nb.value == 16 * 4 * S - sum(
            16 * 2 for s in range(S) if planes["gt"][3, 1, s] == callvcf.GT_VEND)
        check(ctx.L.bcfgpu_memset(ctx.h, buf.ptr, 0xA5, need))
        wide = np.zeros(6, dtype=abi.VCF_FIELD)                                         # six 255-value int32 keys: the bound is passed
        wide["site"], wide["kind"], wide["type"], wide["width"] = 3, callvcf.KEY, 3, 255
        assert callvcf.site_bound(wide, ngmax) > abi.VCF_SAMPLE_CAP >= callvcf.site_bound(wide[:5], ngmax)
        bad(abi.E_ARG, fields=wide, d_indiv=d_in.ptr, n_indiv=2 ** 40)
        bad(abi.E_RANGE, "off", indiv.nbytes, rkey); bad(abi.E_RANGE, "off", 2 ** 63, rkey)
        bad(abi.E_RANGE, n_indiv=int(fields["off"].max()))                               # the last run passes the end
        f = fields.copy()
        plain = int(keys[1])
        assert not f["flags"][plain] & 1
        f["nals"][plain] = 9                                                             # no R key: nals is not looked at
        assert call(buf.ptr, need, fields=f) == 0 and nb.value == need
        assert buf.download(np.zeros(need, np.uint8)).tobytes() == wdata.tobytes()
        np.testing.assert_array_equal(offsets(), woff)


def test_the_result_does_not_depend_on_the_calls_before(twin):
    """Twice around a bcfgpu_call_remap_bcf and a bcfgpu_call_encode_bcf with other inputs (their workspace slots are its
    neighbours), and after a call of its own with another case."""
    S = 65
    case, other = cases(S), cases(S, seed=1)
    kin, kkeys, ksite = jobs(S, seed=1)
    with context(S) as ctx:
        a = run(ctx, case, S)
        ctx.remap_call_bcf(kin, kkeys, S, ksite, col=list(range(S))[::-1])
        P = Planes(ctx, other[2], other[3])
        ctx.encode_call_bcf(P.out, N, other[4], [1, 2, 3])
        run(ctx, other, S, col=list(range(S))[::-1])
        b = run(ctx, case, S)
    check_equal(a, twin(S))
    check_equal(b, twin(S))


def test_abi_mirror_and_symbol():
    from bcftools_amd import lib
    assert C.sizeof(abi.VcfField) == 32 and np.dtype(abi.VCF_FIELD).itemsize == 32 and np.dtype(callvcf.FIELD_DTYPE) == np.dtype(abi.VCF_FIELD)
    assert [f[0] for f in abi.VcfField._fields_] == ["off", "site", "kind", "type", "width", "nals", "flags"]
    assert abi.VcfField.off.offset == 0 and abi.VcfField.site.offset == 8 and abi.VcfField.kind.offset == 12 and abi.VcfField.flags.offset == 28
    assert (abi.VCF_FIELD_GT, abi.VCF_FIELD_PL, abi.VCF_FIELD_GQ, abi.VCF_FIELD_KEY) == (callvcf.GT, callvcf.PL, callvcf.GQ, callvcf.KEY)
    assert (abi.VCF_MAX_FIELDS, abi.VCF_SAMPLE_CAP) == (callvcf.MAX_FIELDS, callvcf.SAMPLE_CAP) == (16, 15360)
    assert hasattr(lib.load(), "bcfgpu_call_encode_vcf")
