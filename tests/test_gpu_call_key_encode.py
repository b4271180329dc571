"""bcfgpu_call_remap_bcf: the integer pass-through FORMAT keys of call records (AD, ADF, ADR, DP, SP, ...) as BCF2 key blocks, made on
the device from the input records' bytes, the sample map and the site records' als_map.  The bytes and all n_keys + 1 offsets are
compared exactly with the numpy twin of tests/helpers/keyenc.py (itself pinned against the host writer and the reference's goldens in
tests/test_call_key_encoder.py).  The shapes are the smallest that reach every branch: 37 records x 3 keys with nals cycling 1..5
and alleles dropped at the front, in the middle, at the end, all but the first, or not at all; 1, 3, 64, 65 and 257 input samples --
one lane, a partial wavefront, one wavefront, one past it, one past the 256-lane workgroup and, for the widest keys, past a slice."""
import ctypes as C

import numpy as np
import pytest

from bcftools_amd import abi, engine, host
from bcftools_amd.lib import check
from tests.helpers import keyenc

pytestmark = pytest.mark.gpu

MISSING, VEND = abi.INT32_MISSING, abi.INT32_VECTOR_END
N = 37
SIZES = [1, 3, 64, 65, 257]
DT = {1: "<i1", 2: "<i2", 3: "<i4"}
SENT = {1: (-128, -127), 2: (-32768, -32767), 3: (MISSING, VEND)}
HI = {1: 100, 2: 30000, 3: 99999}                                   # values below: the input type holds them


def sites(n=N):
    """n site records: nals cycles 1..5; every fifth run of records another way of dropping alleles."""
    site = np.zeros(n, dtype=host.CALLSITE_DTYPE)
    nals = 1 + np.arange(n) % 5
    for r in range(n):
        a, how = int(nals[r]), (r // 5) % 5
        keep = list(range(a))
        if a > 1 and how == 1:
            keep = keep[1:]                                         # the front
        elif a > 2 and how == 2:
            keep = keep[:a // 2] + keep[a // 2 + 1:]                # the middle
        elif a > 1 and how == 3:
            keep = keep[:-1]                                        # the end
        elif a > 1 and how == 4:
            keep = keep[:1]                                         # all but the first: nals_new 1
        m = [-1] * 5
        for new, old in enumerate(keep):
            m[old] = new
        site["nals_new"][r], site["als_map"][r] = len(keep), m
        site["ret"][r] = len(keep)
    return site, nals


def narrow(vals, t):
    """An int64 array with the int32 sentinels -> the bytes of type t."""
    a = np.array(vals, np.int64)
    out = a.copy()
    out[a == MISSING], out[a == VEND] = SENT[t]
    return out.astype(DT[t]).tobytes()


def key_values(rng, S, width, t, sentinels=True):
    """[S][width] values the type holds, with `missing` at the first, a middle and the last position of some samples, a sample that is
    '.' and one with a value too few (when there is room)."""
    v = rng.integers(0, HI[t], (S, width)).astype(np.int64)
    if t > 1:
        v[rng.integers(0, S), rng.integers(0, width)] = HI[t]      # (at least one value the narrower type does not hold)
    if sentinels and width:
        for s, j in ((0, 0), (S // 2, width // 2), (S - 1, width - 1)):
            v[s, j] = MISSING
        if S > 3:
            v[1, 0], v[1, 1:] = MISSING, VEND                       # '.'
            v[S - 2, width - 1:] = VEND                             # one value short (width 1: ends at once, '.')
    return v


def jobs(S, seed=0, n=N):
    """(indiv bytes, keys [3 n] of abi.BCF_KEY, site records).  Per record: an R key with a value per allele, a one-value key, and a
    third that takes the other paths in turn.  Runs start at every byte offset mod 16."""
    rng = np.random.default_rng(1000 * seed + S)
    site, nals = sites(n)
    keys = np.zeros(3 * n, dtype=abi.BCF_KEY)
    buf = bytearray()

    def add(j, r, key_id, t, width, flags, vals):
        while len(buf) % 16 != j % 16:
            buf.append(0xEE)
        keys[j] = (len(buf), r, key_id, t, width, int(nals[r]), flags)
        if t and width:
            buf.extend(narrow(vals, t))

    for r in range(n):
        a = int(nals[r])
        dropped = [i for i in range(a) if site["als_map"][r][i] < 0]
        t = 1 + r % 3
        v = key_values(rng, S, a, t)
        if r % 2 and dropped and t > 1:                             # the only values past the narrower type sit on a dropped allele
            big = v > HI[t - 1]
            v[big] = 7
            v[rng.integers(0, S), dropped[0]] = HI[t]
        add(3 * r, r, 5, t, a, 1, v)
        t = 1 + (r + 1) % 3
        add(3 * r + 1, r, 300 if r % 4 == 0 else 6, t if r % 6 else 0, 1 if r % 9 else 0, r % 2, key_values(rng, S, 1, t))
        kind = r % 7
        if kind == 0:                                               # an R key a value wider than the alleles: left alone
            add(3 * r + 2, r, 9, 2, a + 1, 1, key_values(rng, S, a + 1, 2, sentinels=False))
        elif kind == 1:                                             # 130 values a sample, no R key
            add(3 * r + 2, r, 70000, 1, 130, 0, key_values(rng, S, 130, 1))
        elif kind == 2:                                             # not minimally encoded: int32 holding small values, padded
            v = np.full((S, a + 2), VEND, np.int64)
            v[:, :a] = rng.integers(-100, 100, (S, a))
            add(3 * r + 2, r, 9, 3, a + 2, 1, v)
        elif kind == 3:                                             # every sample missing
            v = np.full((S, a), VEND, np.int64)
            v[:, 0] = MISSING
            add(3 * r + 2, r, 9, 2, a, 1, v)
        elif kind == 4:                                             # negative values at the types' lower bounds
            v = key_values(rng, S, a, 3, sentinels=False)
            v[:] = np.minimum(v, 100)
            v[S // 2, a - 1] = (-120, -121, -32760, -32761)[(r // 7) % 4]
            add(3 * r + 2, r, 9, 3, a, 1, v)
        elif kind == 5:                                             # 255 values of int32: the fewest samples a slice
            add(3 * r + 2, r, 9, 3, 255, 0, key_values(rng, S, 255, 3))
        else:                                                       # 15 values: the long descriptor's first width
            add(3 * r + 2, r, 9, 1, 15, 0, key_values(rng, S, 15, 1))
    buf.extend(b"\xEE" * 3)
    return np.frombuffer(bytes(buf), np.uint8), keys, site


def check_equal(got, exp):
    data, off = got
    wdata, woff = exp
    assert len(off) == len(woff)
    np.testing.assert_array_equal(off, woff)
    assert data.tobytes() == wdata.tobytes()


def context(S, n=N):
    return engine.Context(abi.default_cfg(S, max_sites=max(n, 1), max_reads=64))


@pytest.fixture(scope="module")
def twin():
    """The twin's answer for a case, computed once."""
    memo = {}

    def get(S_in, col=None, emit=None):
        k = (S_in, None if col is None else tuple(col), None if emit is None else tuple(emit))
        if k not in memo:
            indiv, keys, site = jobs(S_in)
            memo[k] = keyenc.encode_jobs(indiv, keys, S_in, site, S_in if col is None else len(col), col, emit)
        return memo[k]
    return get


@pytest.mark.parametrize("S", SIZES)
def test_every_job_at_every_sample_count(S, twin):
    indiv, keys, site = jobs(S)
    assert {int(k["off"]) % 16 for k in keys if k["type"] and k["width"]} == set(range(16))
    with context(S) as ctx:
        got = ctx.remap_call_bcf(indiv, keys, S, site)
    exp = twin(S)
    check_equal(got, exp)
    sizes = np.diff(exp[1].astype(np.int64))
    assert (sizes > 0).all() and len({int(x) % 16 for x in exp[1][:-1]}) > (4 if S == 1 else 10)     # the blocks start at many alignments


def test_types_and_widths_shrink(twin):
    """The twin's blocks of the S = 65 case: types below the input's (the large value sat on a dropped allele; int32 holding small
    values) and widths below the input's (an R key that lost alleles; padding that every sample had)."""
    S = 65
    indiv, keys, site = jobs(S)
    data, off = twin(S)
    narrower = shorter = 0
    for j, k in enumerate(keys):
        b = data[int(off[j]):int(off[j + 1])].tobytes()
        p = 2 if k["key_id"] <= 127 else 3 if k["key_id"] <= 32767 else 5
        t, w = b[p] & 15, b[p] >> 4
        if w == 15:
            w = b[p + 2] if b[p + 1] == 0x11 else b[p + 2] | b[p + 3] << 8
        narrower += bool(k["type"]) and t < k["type"]
        shorter += w < k["width"]
    assert narrower >= 5 and shorter >= 10


@pytest.mark.parametrize("S_in,which", [(65, "reversed"), (65, "three"), (65, "twice"), (257, "reversed"), (257, "three")])
def test_a_sample_map(S_in, which, twin):
    col = {"reversed": list(range(S_in))[::-1], "three": [41, 3, S_in - 1], "twice": [7, 64, 7, 0, 33]}[which]
    indiv, keys, site = jobs(S_in)
    with context(len(col)) as ctx:
        got = ctx.remap_call_bcf(indiv, keys, S_in, site, col=col)
    check_equal(got, twin(S_in, col))


def test_fewer_called_samples_without_a_map(twin):
    """cfg.n_smpl below n_smpl_in and no map: called sample s is input sample s."""
    S_in, S = 65, 3
    indiv, keys, site = jobs(S_in)
    with context(S) as ctx:
        got = ctx.remap_call_bcf(indiv, keys, S_in, site)
    check_equal(got, twin(S_in, list(range(S))))


def test_emit_masks_and_no_keys(twin):
    S = 65
    indiv, keys, site = jobs(S)
    first, last = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    first[0], last[-1] = 1, 1
    with context(S) as ctx:
        for emit in (None, np.zeros(N, np.uint8), np.ones(N, np.uint8), (np.arange(N) % 3 != 1).astype(np.uint8), first, last):
            check_equal(ctx.remap_call_bcf(indiv, keys, S, site, emit=emit), twin(S, None, emit))
        data, off = ctx.remap_call_bcf(indiv, keys[:0], S, site)
        assert len(data) == 0 and off.tolist() == [0]
    assert len(twin(S, None, np.zeros(N, np.uint8))[0]) == 0


def raw_call(ctx, keys, S_in, d_indiv, n_indiv, col, d_site, n_sites, d_emit, d_buf, cap, d_off, nb):
    k = np.ascontiguousarray(keys, dtype=abi.BCF_KEY)
    c = None if col is None else np.ascontiguousarray(col, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    return ctx.L.bcfgpu_call_remap_bcf(ctx.h, len(k), k.ctypes.data_as(C.POINTER(abi.BcfKey)), S_in, d_indiv, n_indiv, c, d_site, n_sites, d_emit,
                                       d_buf, cap, d_off, C.byref(nb))


def test_sizes_and_bad_arguments(twin):
    """The size-only call; cap_bytes one byte short (E_RANGE, *n_bytes the size, nothing written, the offsets set all the same); the
    exact size; then every E_ARG / E_RANGE case, each with nothing written."""
    S = 65
    indiv, keys, site = jobs(S)
    wdata, woff = twin(S)
    need = len(wdata)
    with context(S) as ctx:
        d_in, d_site = ctx.to_device(indiv), ctx.to_device(site.view(np.uint8).reshape(-1))
        buf, off = ctx.buf(need), ctx.buf(8 * (len(keys) + 1))
        nb = C.c_uint64(0)
        args = (S, d_in.ptr, indiv.nbytes, None, d_site.ptr, N, None)

        def untouched():
            return (buf.download(np.zeros(need, np.uint8)) == 0xA5).all()
        check(ctx.L.bcfgpu_memset(ctx.h, buf.ptr, 0xA5, need))
        assert raw_call(ctx, keys, *args, None, 0, off.ptr, nb) == abi.E_RANGE and nb.value == need     # cap_bytes = 0 asks for the size
        np.testing.assert_array_equal(off.download(np.zeros(len(keys) + 1, np.uint64)), woff)
        check(ctx.L.bcfgpu_memset(ctx.h, off.ptr, 0, 8 * (len(keys) + 1)))
        assert raw_call(ctx, keys, *args, buf.ptr, need - 1, off.ptr, nb) == abi.E_RANGE and nb.value == need and untouched()
        np.testing.assert_array_equal(off.download(np.zeros(len(keys) + 1, np.uint64)), woff)
        with pytest.raises(engine.BcfGpuError) as e:
            ctx.remap_call_bcf(indiv, keys, S, site, cap_bytes=need - 1)
        assert e.value.code == abi.E_RANGE and e.value.needed == need

        def bad(code, field=None, value=None, j=5, **kw):
            k = keys.copy()
            if field:
                k[field][j] = value
            a = dict(zip(("S_in", "d_indiv", "n_indiv", "col", "d_site", "n_sites", "d_emit"), args))
            a.update(kw)
            nb.value = 12345
            rc = raw_call(ctx, k, a["S_in"], a["d_indiv"], a["n_indiv"], a["col"], a["d_site"], a["n_sites"], a["d_emit"],
                          a.get("d_buf", buf.ptr), need, a.get("d_off", off.ptr), nb)
            assert rc == code and nb.value == 0 and untouched(), (field, value, kw)
        bad(abi.E_ARG, "type", 4); bad(abi.E_ARG, "type", -1); bad(abi.E_ARG, "type", 5)
        bad(abi.E_ARG, "width", -1); bad(abi.E_ARG, "width", 256)
        bad(abi.E_ARG, "site", -1); bad(abi.E_ARG, "site", N)
        bad(abi.E_ARG, "key_id", -1)
        bad(abi.E_ARG, "nals", 0, j=3); bad(abi.E_ARG, "nals", 6, j=3)                              # (job 3 is an R key)
        bad(abi.E_ARG, col=[0] * (S - 1) + [S]); bad(abi.E_ARG, col=[-1] + [0] * (S - 1))
        bad(abi.E_ARG, d_site=None); bad(abi.E_ARG, d_off=None); bad(abi.E_ARG, d_buf=None); bad(abi.E_ARG, d_indiv=None)
        bad(abi.E_ARG, S_in=0); bad(abi.E_ARG, S_in=S - 1)                                           # more called samples than input samples
        assert ctx.L.bcfgpu_call_remap_bcf(ctx.h, len(keys), None, *args, buf.ptr, need, off.ptr, C.byref(nb)) == abi.E_ARG and untouched()
        assert ctx.L.bcfgpu_call_remap_bcf(ctx.h, len(keys), keys.ctypes.data_as(C.POINTER(abi.BcfKey)), *args, buf.ptr, need, off.ptr, None) == abi.E_ARG
        assert untouched()
        bad(abi.E_RANGE, "off", indiv.nbytes, j=3); bad(abi.E_RANGE, "off", 2 ** 63, j=3)
        bad(abi.E_RANGE, n_indiv=int(keys["off"].max()))                                             # the last run passes the end
        k = keys.copy()
        assert not k["flags"][1] & 1
        k["nals"][1] = 9                                                                             # no R key: nals is not looked at
        assert raw_call(ctx, k, *args, buf.ptr, need, off.ptr, nb) == 0 and nb.value == need
        assert buf.download(np.zeros(need, np.uint8)).tobytes() == wdata.tobytes()
        np.testing.assert_array_equal(off.download(np.zeros(len(keys) + 1, np.uint64)), woff)


def test_the_result_does_not_depend_on_the_calls_before(twin):
    """Twice around a bcfgpu_call_decode_bcf (whose workspace slots are its neighbours), and after a call with other jobs."""
    S = 65
    indiv, keys, site = jobs(S)
    other = jobs(S, seed=1)
    with context(S) as ctx:
        a = ctx.remap_call_bcf(indiv, keys, S, site)
        ctx.decode_bcf(indiv, [(int(k["off"]), int(k["type"]), int(k["width"])) for k in keys[:9]], S, 5)
        ctx.remap_call_bcf(other[0], other[1][::-1].copy(), S, other[2], col=list(range(S))[::-1])
        b = ctx.remap_call_bcf(indiv, keys, S, site)
    check_equal(a, twin(S))
    check_equal(b, twin(S))


def test_abi_mirror_and_symbol():
    from bcftools_amd import lib
    assert C.sizeof(abi.BcfKey) == 32 and np.dtype(abi.BCF_KEY).itemsize == 32 and np.dtype(keyenc.KEY_DTYPE) == np.dtype(abi.BCF_KEY)
    assert [f[0] for f in abi.BcfKey._fields_] == ["off", "site", "key_id", "type", "width", "nals", "flags"]
    assert abi.BcfKey.off.offset == 0 and abi.BcfKey.site.offset == 8 and abi.BcfKey.flags.offset == 28
    assert hasattr(lib.load(), "bcfgpu_call_remap_bcf")
