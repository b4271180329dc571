"""bcfgpu_call_parse_keys_vcf: the integer pass-through FORMAT keys of call records of VCF text input (AD, ADF, ADR, DP, SP, ...) as BCF2
key blocks, made on the device from the input records' own sample columns, the sample map and the site records' als_map.  The bytes,
all n_keys + 1 offsets and the n_keys status bytes are compared exactly with the twin of tests/helpers/keytext.py (itself pinned
against the host writer and the reference's goldens in tests/test_call_key_text_encoder.py).  The shapes are those of
tests/test_gpu_call_key_encode.py, the smallest that reach every branch: 37 records x 3 keys with nals cycling 1..5 and alleles
dropped at the front, in the middle, at the end, all but the first, or not at all; 1, 3, 64, 65 and 257 input samples -- one lane, a
partial wavefront, one wavefront, one past it, one past the 256-lane workgroup.  One column is longer than the 15 360 bytes of a
stage, the columns of some records cut a round by bytes on the input side, a 255-value int32 key cuts it on the output side."""
import ctypes as C

import numpy as np
import pytest

from bcftools_amd import abi, engine
from bcftools_amd.lib import check
from tests.helpers import keytext
from tests.helpers.callvcftextgen import cases as rewrite_cases
from tests.test_gpu_call_key_encode import HI, N, SIZES, context, sites
from tests.test_gpu_call_key_encode import jobs as bcf_jobs
from tests.test_gpu_call_vcf_encode import Planes

pytestmark = pytest.mark.gpu

STAGE = 15360
BAD = ["", "12x", " 5", "2147483648", "-2147483649", "99999999999", "+", "3,,4"]
_JUNK = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789,;=|/._-+ ", np.uint8)


def number(rng, v):
    """v in one of the spellings the grammar allows."""
    how = int(rng.integers(0, 8))
    return "+%d" % v if how == 0 and v >= 0 else "%s00%d" % ("-" if v < 0 else "", abs(v)) if how == 1 else "%d" % v


def vector(rng, width, hi, lo=0):
    return [number(rng, int(x)) for x in rng.integers(lo, hi, width)]


def jobs(S, seed=0, n=N):
    """(text bytes, runs [n] of abi.VCF_VEC, keys [3 n] of abi.VCF_KEY, site records).  A column is junk : R key : one-value key : third
    key; per record the third key takes the other paths in turn.  Runs start at every byte offset mod 16."""
    rng = np.random.default_rng(1000 * seed + S + 77)
    site, nals = sites(n)
    keys = np.zeros(3 * n, dtype=abi.VCF_KEY)
    run = np.zeros(n, dtype=abi.VCF_VEC)
    buf = bytearray()
    for r in range(n):
        a = int(nals[r])
        dropped = [i for i in range(a) if site["als_map"][r][i] < 0]
        t = 1 + r % 3
        kind = r % 8
        junk_len = (100, 300) if r % 4 == 2 else (0, 12)        # (r % 4 == 2: 256 columns are past a stage: rounds cut by bytes)
        big_on_dropped = r % 2 and dropped and t > 1
        cols = []
        for s in range(S):
            tok = ["".join(map(chr, rng.choice(_JUNK, int(rng.integers(*junk_len) if junk_len[0] else rng.integers(0, 12)))))]
            if r == 10 and s == S // 2:
                tok[0] = "".join(map(chr, rng.choice(_JUNK, STAGE + 500)))      # one column longer than the stage
            # the R key: a value per allele; the only values past the narrower type on a dropped allele in every other record
            v = vector(rng, a, HI[t - 1] if big_on_dropped else HI[t])
            if big_on_dropped and s == S // 3:
                v[dropped[0]] = "%d" % HI[t]
            if not big_on_dropped and t > 1 and s == S // 3:
                v[a - 1] = "%d" % HI[t]
            if s % 11 == 3:
                v[int(rng.integers(0, a))] = "."
            tok.append(",".join(v))
            if S > 3 and s == 2:
                tok[1] = "."                                    # '.' beside samples with a value per allele
            if S > 3 and s == S - 1 and a > 1:
                tok[1] = ",".join(v[:-1])                       # one value short: left alone
            # the one-value key
            tok.append("." if (r % 9 == 0 or s % 13 == 5) else number(rng, int(rng.integers(0, HI[1 + (r + 1) % 3]))))
            # the third key
            if kind == 0:                                       # an R key a value wider than the alleles: left alone
                tok.append(",".join(vector(rng, a + 1, 30000)))
            elif kind == 1:                                     # 130 values a sample
                tok.append(",".join(vector(rng, 130, 100)))
            elif kind == 2:                                     # every sample missing (and some of them by a column that ends early)
                tok.append(".")
            elif kind == 3:                                     # negative values at the types' lower bounds
                v = vector(rng, a, 100, -100)
                if s == S // 2:
                    v[a - 1] = "%d" % (-120, -121, -32760, -32761)[(r // 8) % 4]
                tok.append(",".join(v))
            elif kind == 4:                                     # 255 values of int32: the fewest samples a round on the output side
                v = vector(rng, 255 if s % 2 == 0 else 17, 10)
                if s == 0:
                    v[254] = "70000"
                tok.append(",".join(v))
            elif kind == 5:                                     # 15 values: the long descriptor's first width
                tok.append(",".join(vector(rng, 15, 100)))
            elif kind == 6:                                     # a value outside the grammar in one sample: status 1
                v = vector(rng, a, 100)
                if s == S // 2:
                    v[int(rng.integers(0, a))] = BAD[(r // 8) % 4]
                elif s == 0 and r % 16 == 6:
                    v[int(rng.integers(0, a))] = BAD[4 + (r // 16) % 4]
                tok.append(",".join(v))
            else:                                               # 256 values in one sample: status 2; the sentinels' texts in the others
                v = vector(rng, 256, 10) if s == S - 1 else ["1", "-2147483648", "-2147483647", "4"]
                tok.append(",".join(v))
            if S > 3 and s == 1:
                tok = ["."]                                     # a whole-column '.'
            if S > 3 and s == S - 2 and kind not in (4, 7):
                tok = tok[:3] if r % 2 else tok[:2]             # a column shorter than idx
            cols.append(":".join(tok))
        while len(buf) % 16 != r % 16:
            buf.append(0xEE)
        text = "".join("\t" + c for c in cols).encode("latin-1")
        run[r] = (len(buf), len(text), -7)
        buf.extend(text)
        keys[3 * r] = (r, (5, 300, 70000)[r % 3], 1, a, 1, 0)
        keys[3 * r + 1] = (r, 300 if r % 4 == 0 else 6, 2, a, r % 2, 0)
        keys[3 * r + 2] = (r, (9, 70000, 400)[(r // 2) % 3], 63 if r == 2 else 3, a, int(kind in (0, 3, 6)), 0)
    buf.extend(b"\xEE" * 3)
    return np.frombuffer(bytes(buf), np.uint8), run, keys, site


def check_equal(got, exp):
    data, off, status = got
    wdata, woff, wstatus = exp
    assert len(off) == len(woff) and len(status) == len(wstatus)
    np.testing.assert_array_equal(status, wstatus)
    np.testing.assert_array_equal(off, woff)
    assert data.tobytes() == wdata.tobytes()


@pytest.fixture(scope="module")
def twin():
    """The twin's answer for a case, computed once."""
    memo = {}

    def get(S_in, col=None, emit=None):
        k = (S_in, None if col is None else tuple(col), None if emit is None else tuple(emit))
        if k not in memo:
            text, run, keys, site = jobs(S_in)
            memo[k] = keytext.encode_jobs(text, run, keys, S_in, site, S_in if col is None else len(col), col, emit)
        return memo[k]
    return get


@pytest.mark.parametrize("S", SIZES)
def test_every_job_at_every_sample_count(S, twin):
    text, run, keys, site = jobs(S)
    assert {int(r["off"]) % 16 for r in run} == set(range(16))
    with context(S) as ctx:
        got = ctx.parse_keys_vcf(text, keys, run, S, site)
    exp = twin(S)
    check_equal(got, exp)
    sizes, status = np.diff(exp[1].astype(np.int64)), exp[2]
    assert ((sizes > 0) == (status == 0)).all() and set(status.tolist()) == {0, 1, 2}
    # a flagged job lies between good ones, and the blocks start at every alignment (the key ids and widths in front differ)
    assert all(status[j - 1] == 0 and status[j - 2] == 0 for j in np.flatnonzero(status))
    assert {int(x) % 16 for x in exp[1][:-1]} == set(range(16))
    if S >= 65:                                                     # more than one round by bytes, on either side
        assert int(run["len"].max()) > (2 * STAGE if S > 256 else STAGE) and sizes.max() > STAGE
        assert max(len(c) for c in bytes(text[int(run["off"][10]):int(run["off"][10]) + int(run["len"][10])]).split(b"\t")) > STAGE


def test_types_and_widths_follow_the_output(twin):
    """The twin's blocks of the S = 65 case: int8 blocks of R keys whose text holds values past int8 (they sat on a dropped allele),
    widths below the alleles of the input, every type and both descriptor forms."""
    S = 65
    text, run, keys, site = jobs(S)
    data, off, status = twin(S)
    types, widths, narrowed = set(), set(), 0
    for j, k in enumerate(keys):
        b = data[int(off[j]):int(off[j + 1])].tobytes()
        if not b:
            continue
        p = 2 if k["key_id"] <= 127 else 3 if k["key_id"] <= 32767 else 5
        t, w = b[p] & 15, b[p] >> 4
        if w == 15:
            w = b[p + 2] if b[p + 1] == 0x11 else b[p + 2] | b[p + 3] << 8
        types.add(t); widths.add(w)
        r = int(k["site"])
        narrowed += j % 3 == 0 and t < 1 + r % 3
    assert types == {1, 2, 3} and {1, 2, 3, 4, 5, 15, 130, 255} <= widths and narrowed >= 3


@pytest.mark.parametrize("S_in,which", [(65, "reversed"), (65, "three"), (65, "twice"), (257, "reversed"), (257, "three")])
def test_a_sample_map(S_in, which, twin):
    col = {"reversed": list(range(S_in))[::-1], "three": [41, 3, S_in - 1], "twice": [7, 64, 7, 0, 33]}[which]
    text, run, keys, site = jobs(S_in)
    with context(len(col)) as ctx:
        got = ctx.parse_keys_vcf(text, keys, run, S_in, site, col=col)
    check_equal(got, twin(S_in, col))


def test_an_identity_map_gives_the_same_bytes(twin):
    S = 65
    text, run, keys, site = jobs(S)
    with context(S) as ctx:
        check_equal(ctx.parse_keys_vcf(text, keys, run, S, site, col=list(range(S))), twin(S))


def test_fewer_called_samples_without_a_map(twin):
    """cfg.n_smpl below n_smpl_in and no map: called sample s is input column s; the columns of the others are not examined (the
    256-value column and the malformed values of the samples past the third are not seen: only the jobs with a bad value in sample 0
    stay flagged)."""
    S_in, S = 65, 3
    text, run, keys, site = jobs(S_in)
    with context(S) as ctx:
        got = ctx.parse_keys_vcf(text, keys, run, S_in, site)
    exp = twin(S_in, list(range(S)))
    check_equal(got, exp)
    assert set(exp[2].tolist()) == {0, 1} and 0 < int((exp[2] != 0).sum()) < int((twin(S_in)[2] == 1).sum())


def test_emit_masks_and_no_keys(twin):
    S = 65
    text, run, keys, site = jobs(S)
    first, last = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    first[0], last[-1] = 1, 1
    with context(S) as ctx:
        for emit in (None, np.zeros(N, np.uint8), np.ones(N, np.uint8), (np.arange(N) % 3 != 1).astype(np.uint8), first, last):
            check_equal(ctx.parse_keys_vcf(text, keys, run, S, site, emit=emit), twin(S, None, emit))
        data, off, status = ctx.parse_keys_vcf(text, keys[:0], run, S, site)
        assert len(data) == 0 and off.tolist() == [0] and len(status) == 0
        # a site without a record is not indexed: its run may be anything inside the text
        odd = run.copy()
        odd["off"][4] += 1
        emit = (np.arange(N) != 4).astype(np.uint8)
        check_equal(ctx.parse_keys_vcf(text, keys, odd, S, site, emit=emit), twin(S, None, emit))
    assert len(twin(S, None, np.zeros(N, np.uint8))[0]) == 0 and (twin(S, None, np.zeros(N, np.uint8))[2] == 0).all()


def test_more_sites_than_a_chunk_of_column_offsets():
    """The columns' offsets of all sites do not fit the workspace: the kernels run over chunks of sites, the indexing kernel before each."""
    S = 257
    fits = abi.VCFDEC_START_BYTES // 4 // (S + 1)
    n = fits + 200
    cols = ["%d,%d:%d" % (s, s % 7, 200 + s) for s in range(S)]
    one = "".join("\t" + c for c in cols).encode()
    text = np.frombuffer(one * 2, np.uint8)                         # every site reads one of two copies
    run = np.zeros(n, dtype=abi.VCF_VEC)
    run["off"], run["len"] = (np.arange(n) % 2) * len(one), len(one)
    site = np.zeros(n, dtype=sites(1)[0].dtype)
    site["nals_new"], site["als_map"] = 1 + np.arange(n) % 2, [0, 1, -1, -1, -1]
    emit = (np.arange(n) % 50 != 7).astype(np.uint8)
    assert int(emit.sum()) > fits                                   # the sites with a record alone are more than a chunk
    keys = np.zeros(2 * n, dtype=abi.VCF_KEY)
    keys["site"], keys["key_id"], keys["idx"], keys["nals"], keys["flags"] = np.repeat(np.arange(n), 2), [5, 6] * n, [0, 1] * n, 2, [1, 0] * n
    exp = keytext.encode_jobs(text, run[:4], keys[:8], S, site[:4], S, emit=[1, 1, 1, 1])
    a, b = exp[0][:int(exp[1][2])].tobytes(), exp[0][int(exp[1][2]):int(exp[1][4])].tobytes()    # a site that lost an allele, one that did not
    with context(S, n) as ctx:
        data, off, status = ctx.parse_keys_vcf(text, keys, run, S, site, emit=emit)
    assert (status == 0).all()
    want = b"".join((a if k % 2 == 0 else b) if emit[k] else b"" for k in range(n))
    assert data.tobytes() == want and int(off[-1]) == len(want)
    sizes = np.diff(off.astype(np.int64)).reshape(n, 2).sum(1)
    np.testing.assert_array_equal(sizes, np.where(emit, np.where(np.arange(n) % 2 == 0, len(a), len(b)), 0))


def raw_call(ctx, keys, n_sites, run, S_in, d_text, n_text, col, d_site, d_emit, d_buf, cap, d_off, nb, status):
    k = None if keys is None else np.ascontiguousarray(keys, dtype=abi.VCF_KEY)
    r = None if run is None else np.ascontiguousarray(run, dtype=abi.VCF_VEC)
    c = None if col is None else np.ascontiguousarray(col, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    return ctx.L.bcfgpu_call_parse_keys_vcf(ctx.h, 0 if k is None else len(k), None if k is None else k.ctypes.data_as(C.POINTER(abi.VcfKey)), n_sites,
                                            None if r is None else r.ctypes.data_as(C.POINTER(abi.VcfVec)), S_in, d_text, n_text, c, d_site, d_emit,
                                            d_buf, cap, d_off, None if nb is None else C.byref(nb), None if status is None else status.ctypes.data)


def test_sizes_and_bad_arguments(twin):
    """The size-only call; cap_bytes one byte short (E_RANGE, *n_bytes the size, the offsets and the status set all the same, and a
    guard band around d_buf untouched); the exact size inside the guard band; then every E_ARG / E_RANGE case, each with nothing written."""
    S = 65
    text, run, keys, site = jobs(S)
    wdata, woff, wstatus = twin(S)
    need, front, back, n_off = len(wdata), 61, 4096, len(keys) + 1
    with context(S) as ctx:
        d_text, d_site = ctx.to_device(text), ctx.to_device(site.view(np.uint8).reshape(-1))
        whole, off = ctx.buf(front + need + back), ctx.buf(8 * n_off)
        buf = whole.ptr + front
        nb, status = C.c_uint64(0), np.full(len(keys), 9, np.uint8)
        args = dict(keys=keys, n_sites=N, run=run, S_in=S, d_text=d_text.ptr, n_text=text.nbytes, col=None, d_site=d_site.ptr, d_emit=None)

        def untouched():
            return (whole.download(np.zeros(front + need + back, np.uint8)) == 0xA5).all()
        check(ctx.L.bcfgpu_memset(ctx.h, whole.ptr, 0xA5, front + need + back))
        assert raw_call(ctx, **args, d_buf=None, cap=0, d_off=off.ptr, nb=nb, status=status) == abi.E_RANGE and nb.value == need     # cap_bytes = 0 asks for the size
        np.testing.assert_array_equal(off.download(np.zeros(n_off, np.uint64)), woff)
        np.testing.assert_array_equal(status, wstatus)
        check(ctx.L.bcfgpu_memset(ctx.h, off.ptr, 0, 8 * n_off))
        status[:] = 9
        assert raw_call(ctx, **args, d_buf=buf, cap=need - 1, d_off=off.ptr, nb=nb, status=status) == abi.E_RANGE and nb.value == need and untouched()
        np.testing.assert_array_equal(off.download(np.zeros(n_off, np.uint64)), woff)
        np.testing.assert_array_equal(status, wstatus)
        with pytest.raises(engine.BcfGpuError) as e:
            ctx.parse_keys_vcf(text, keys, run, S, site, cap_bytes=need - 1)
        assert e.value.code == abi.E_RANGE and e.value.needed == need and e.value.status.tolist() == wstatus.tolist()

        def bad(code, field=None, value=None, j=5, **kw):
            a = dict(args, d_buf=buf, cap=need, d_off=off.ptr, nb=nb, status=status)
            if field:
                a["keys"] = keys.copy()
                if field.startswith("reserved"):
                    a["keys"]["reserved"][j][int(field[-1])] = value
                else:
                    a["keys"][field][j] = value
            a.update(kw)
            nb.value = 12345
            assert raw_call(ctx, **a) == code and (nb.value == 0 or a["nb"] is None) and untouched(), (field, value, kw)
        bad(abi.E_ARG, "site", -1); bad(abi.E_ARG, "site", N); bad(abi.E_ARG, "site", 0)              # (job 5's site is 1: the sites decrease)
        bad(abi.E_ARG, "site", 3, j=3)
        bad(abi.E_ARG, "key_id", -1)
        bad(abi.E_ARG, "idx", -1); bad(abi.E_ARG, "idx", abi.VCF_REWRITE_MAX_KEYS)
        bad(abi.E_ARG, "nals", 0, j=3); bad(abi.E_ARG, "nals", 6, j=3)                              # (job 3 is an R key)
        bad(abi.E_ARG, "reserved0", 1); bad(abi.E_ARG, "reserved1", -1); bad(abi.E_ARG, "reserved2", 7)
        bad(abi.E_ARG, col=[0] * (S - 1) + [S]); bad(abi.E_ARG, col=[-1] + [0] * (S - 1))
        bad(abi.E_ARG, S_in=0); bad(abi.E_ARG, S_in=S - 1)                                           # more called samples than input samples
        bad(abi.E_ARG, d_site=None); bad(abi.E_ARG, d_off=None); bad(abi.E_ARG, d_buf=None); bad(abi.E_ARG, d_text=None)
        bad(abi.E_ARG, run=None); bad(abi.E_ARG, status=None); bad(abi.E_ARG, nb=None)
        assert raw_call(ctx, **dict(args, keys=None), d_buf=buf, cap=need, d_off=off.ptr, nb=nb, status=status) == 0 and nb.value == 0       # (no keys: n_keys == 0)
        assert ctx.L.bcfgpu_call_parse_keys_vcf(ctx.h, len(keys), None, N, run.ctypes.data_as(C.POINTER(abi.VcfVec)), S, d_text.ptr, text.nbytes, None, d_site.ptr, None,
                                                buf, need, off.ptr, C.byref(nb), status.ctypes.data) == abi.E_ARG and untouched()
        # found by the indexing pass: a run that does not start at a tab, a run with a tab too few, a column count that is not the input's
        for k, d_off_, d_len in ((7, 1, -1), (7, 0, -(int(run["len"][7]) // 2)), (N - 1, 1, -1)):
            r = run.copy()
            r["off"][k] += d_off_
            r["len"][k] = int(r["len"][k]) + d_len
            bad(abi.E_ARG, run=r)
        bad(abi.E_ARG, S_in=S + 1)
        r = run.copy()
        r["off"][7] += 1
        emit = ctx.to_device((np.arange(N) != 7).astype(np.uint8))
        nb.value = 0
        assert raw_call(ctx, **dict(args, run=r, d_emit=emit.ptr), d_buf=None, cap=0, d_off=off.ptr, nb=nb, status=status) == abi.E_RANGE and nb.value > 0    # (not indexed)
        # E_RANGE: a run past the end of the text, a run past 1 GiB
        r = run.copy()
        r["len"][N - 1] += 4
        bad(abi.E_RANGE, run=r)
        r = run.copy()
        r["off"][0] = 2 ** 63
        bad(abi.E_RANGE, run=r)
        bad(abi.E_RANGE, n_text=int(run["off"][N - 1]) + int(run["len"][N - 1]) - 1)
        r = run.copy()
        r["off"][3], r["len"][3] = 0, 2 ** 30 + 1
        bad(abi.E_RANGE, run=r, n_text=2 ** 31)
        k = keys.copy()
        assert not k["flags"][1] & 1
        k["nals"][1] = 9                                                                             # no R key: nals is not looked at
        status[:] = 9
        assert raw_call(ctx, **dict(args, keys=k), d_buf=buf, cap=need, d_off=off.ptr, nb=nb, status=status) == 0 and nb.value == need
        got = whole.download(np.zeros(front + need + back, np.uint8))
        assert got[front:front + need].tobytes() == wdata.tobytes() and (got[:front] == 0xA5).all() and (got[front + need:] == 0xA5).all()
        np.testing.assert_array_equal(off.download(np.zeros(n_off, np.uint64)), woff)
        np.testing.assert_array_equal(status, wstatus)


def test_the_result_does_not_depend_on_the_calls_before(twin):
    """Twice around a bcfgpu_call_rewrite_vcf and a bcfgpu_call_remap_bcf (they share the scan workspace and the pinned word; their slots
    are its neighbours), and after a call with other jobs."""
    S = 65
    text, run, keys, site = jobs(S)
    other = jobs(S, seed=1)
    rw = rewrite_cases(S)
    kb = bcf_jobs(S, seed=1)
    with context(S, max(N, len(rw[2]))) as ctx:
        a = ctx.parse_keys_vcf(text, keys, run, S, site)
        P = Planes(ctx, rw[2], rw[3])
        ctx.rewrite_call_vcf(P.out, len(rw[2]), rw[4], rw[1], S, rw[0])
        ctx.remap_call_bcf(kb[0], kb[1], S, kb[2])
        ctx.parse_keys_vcf(other[0], other[2], other[1], S, other[3], col=list(range(S))[::-1])
        b = ctx.parse_keys_vcf(text, keys, run, S, site)
    check_equal(a, twin(S))
    check_equal(b, twin(S))


def test_abi_mirror_and_symbol():
    from bcftools_amd import lib
    assert C.sizeof(abi.VcfKey) == 32 and np.dtype(abi.VCF_KEY).itemsize == 32 and np.dtype(keytext.KEY_DTYPE) == np.dtype(abi.VCF_KEY)
    assert [f[0] for f in abi.VcfKey._fields_] == ["site", "key_id", "idx", "nals", "flags", "reserved"]
    assert abi.VcfKey.site.offset == 0 and abi.VcfKey.flags.offset == 16 and abi.VcfKey.reserved.offset == 20
    assert np.dtype(keytext.RUN_DTYPE) == np.dtype(abi.VCF_VEC) and keytext.MAX_KEYS == abi.VCF_REWRITE_MAX_KEYS and keytext.MAX_WIDTH == abi.BCF_KEY_MAX_WIDTH
    assert hasattr(lib.load(), "bcfgpu_call_parse_keys_vcf")
