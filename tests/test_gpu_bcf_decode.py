"""bcfgpu_call_decode_bcf: one FORMAT key's vectors of BCF records, as they lie in the records' per-sample bytes in HBM, as the
int32 planes of bcfgpu_call_in.  The bytes are made by hand (tests/helpers/bcfdec.pack) and the planes compared exactly with
the numpy decoder of tests/helpers/bcfdec.py (itself pinned against the text route in tests/test_bcf_indiv_decoder.py).  The
shapes are the smallest that reach every branch: one lane, a partial wavefront, one wavefront, one past it, past a 256-lane
workgroup; every PL width in every integer type; runs that start at every byte of a 16-byte line; a run larger than a CU's
LDS (several slices, with and without a sample map); a sample wider than the stage.  Every call writes into a buffer with a
patterned tail, which must stay as it was."""
import ctypes as C

import numpy as np
import pytest

from bcftools_amd import abi, engine
from bcftools_amd.lib import check
from tests.helpers import bcfdec
from tests.helpers.bcfdec import MISSING, VEND

pytestmark = pytest.mark.gpu

TAIL = 4096
PATTERN = 0xA5
HI = {1: 127, 2: 32767, 3: 2147483647}


def call(ctx, indiv, vec, n_smpl_in, n_planes, col=None, n_indiv_bytes=None):
    """The C entry on a patterned output buffer: (return code, planes [n, n_planes, S] as they are afterwards).  The tail
    behind the planes is checked here."""
    S, n = ctx.cfg.n_smpl, len(vec)
    raw = np.frombuffer(bytes(indiv), np.uint8)
    v = np.zeros(n, dtype=abi.BCF_VEC)
    if n:
        v["off"], v["type"], v["width"] = [[int(x[i]) for x in vec] for i in range(3)]
    c = None if col is None else np.ascontiguousarray(col, np.int32)
    nb = n * n_planes * S * 4
    d_in, d_out = ctx.to_device(raw), ctx.buf(nb + TAIL)
    check(ctx.L.bcfgpu_memset(ctx.h, d_out.ptr, PATTERN, nb + TAIL))
    rc = ctx.L.bcfgpu_call_decode_bcf(ctx.h, n, n_smpl_in, d_in.ptr, len(raw) if n_indiv_bytes is None else n_indiv_bytes,
                                      v.ctypes.data_as(C.POINTER(abi.BcfVec)), None if c is None else c.ctypes.data_as(C.POINTER(C.c_int32)),
                                      n_planes, d_out.ptr)
    back = d_out.download(np.zeros(nb + TAIL, np.uint8))
    ctx.release([d_in, d_out])
    assert (back[nb:] == PATTERN).all(), "the bytes behind the planes were written"
    return rc, back[:nb].view(np.int32).reshape(n, n_planes, S)


def decode(ctx, indiv, vec, n_smpl_in, n_planes, col=None):
    rc, got = call(ctx, indiv, vec, n_smpl_in, n_planes, col)
    assert rc == 0, ctx.L.bcfgpu_last_error()
    return got


def values(rng, n_smpl_in, width, ty, sentinels=0.05):
    """[n_smpl_in, width] plain values over the type's range with a few `missing` and `end of vector` among them."""
    a = rng.integers(-HI[ty] + 1, HI[ty], (n_smpl_in, width), dtype=np.int64, endpoint=True)
    r = rng.random(a.shape)
    return np.where(r < sentinels / 2, MISSING, np.where(r < sentinels, VEND, a))


def blocks(rng, runs, align=lambda k: k % 16):
    """The records' blocks back to back: every run (bytes) between the bytes of other keys, run k starting at byte
    align(k) of a 16-byte line.  Returns (bytes, [offset of each run])."""
    buf, offs = bytearray(), []
    for k, run in enumerate(runs):
        pad = (align(k) - len(buf)) % 16 + 16 * (k % 2)
        buf += rng.integers(0, 256, pad, dtype=np.uint8).tobytes()
        offs.append(len(buf))
        buf += run
        buf += rng.integers(0, 256, 1 + 2 * int(rng.integers(0, 8)), dtype=np.uint8).tobytes()     # an odd number of bytes behind it
    return bytes(buf), offs


@pytest.mark.parametrize("n_smpl_in", [1, 3, 64, 65, 257])
def test_every_width_type_and_alignment(n_smpl_in):
    """37 records, widths cycling 1, 3, 6, 10, 15 and types int8, int16, int32 (every pair: 15 records), the runs at every
    byte of a line; n_planes = 15 and, clipping the wider vectors, 6."""
    rng = np.random.default_rng(n_smpl_in)
    n = 37
    shape = [((1, 3, 6, 10, 15)[k % 5], 1 + k % 3) for k in range(n)]
    assert len(set(shape)) == 15
    buf, offs = blocks(rng, [bcfdec.pack(values(rng, n_smpl_in, w, t), t) for w, t in shape])
    vec = [(o, t, w) for o, (w, t) in zip(offs, shape)]
    assert {o % 16 for o in offs} == set(range(16))
    assert {(o % 16, t) for o, (w, t) in zip(offs, shape)} >= {(1, 2), (2, 3), (4, 2), (0, 1)}      # values astride their alignment and not
    with engine.Context(abi.default_cfg(n_smpl_in, max_sites=n, max_reads=64)) as ctx:
        for n_planes in (15, 6):
            np.testing.assert_array_equal(decode(ctx, buf, vec, n_smpl_in, n_planes), bcfdec.decode_vec(buf, vec, n_smpl_in, n_planes))
        np.testing.assert_array_equal(ctx.decode_bcf(buf, vec, n_smpl_in, 15), bcfdec.decode_vec(buf, vec, n_smpl_in, 15))


def test_sentinels_at_every_position_in_single_samples():
    """A `missing` and an `end of vector` at the first, a middle and the last position of a width-6 vector, in the first, a
    middle and the last sample only, per type; everything else plain values."""
    S, w = 65, 6
    rng = np.random.default_rng(7)
    cases = [(t, sen, j, s) for t in (1, 2, 3) for sen in (MISSING, VEND) for j in (0, 3, 5) for s in (0, 32, 64)]
    runs = []
    for t, sen, j, s in cases:
        a = values(rng, S, w, t, sentinels=0)
        a[s, j] = sen
        runs.append(bcfdec.pack(a, t))
    buf, offs = blocks(rng, runs, align=lambda k: (3 * k) % 16)
    vec = [(o, t, w) for o, (t, _, _, _) in zip(offs, cases)]
    want = bcfdec.decode_vec(buf, vec, S, w)
    for k, (t, sen, j, s) in enumerate(cases):                  # the yardstick itself, on these cases
        assert want[k, j, s] == (MISSING if j == 0 else sen)
        assert (want[k, j + 1:, s] == VEND).all() == (sen == VEND) or j == w - 1
        assert ((want[k] == MISSING) | (want[k] == VEND)).sum() == (w - j if sen == VEND else 1)
    with engine.Context(abi.default_cfg(S, max_sites=len(cases), max_reads=64)) as ctx:
        np.testing.assert_array_equal(decode(ctx, buf, vec, S, w), want)


@pytest.mark.parametrize("col", [None, list(range(65))[::-1], [64, 7], [5, 5]], ids=["all", "reversed", "two", "twice"])
def test_sample_maps(col):
    n_in, n = 65, 15
    rng = np.random.default_rng(11)
    shape = [((1, 3, 6, 10, 15)[k % 5], 1 + k % 3) for k in range(n)]
    buf, offs = blocks(rng, [bcfdec.pack(values(rng, n_in, w, t), t) for w, t in shape], align=lambda k: (7 * k + 1) % 16)
    vec = [(o, t, w) for o, (w, t) in zip(offs, shape)]
    S = n_in if col is None else len(col)
    with engine.Context(abi.default_cfg(S, max_sites=n, max_reads=64)) as ctx:
        got = decode(ctx, buf, vec, n_in, 15, col)
        np.testing.assert_array_equal(got, bcfdec.decode_vec(buf, vec, n_in, 15, col))
        if col is not None:
            np.testing.assert_array_equal(ctx.decode_bcf(buf, vec, n_in, 15, col=col), got)
    assert got.shape == (n, 15, S)


def test_records_without_the_key_and_without_values_among_ordinary_ones():
    S = 65
    rng = np.random.default_rng(13)
    runs = [bcfdec.pack(values(rng, S, 3, 1 + k % 3), 1 + k % 3) for k in range(9)]
    buf, offs = blocks(rng, runs)
    vec = [(o, 1 + k % 3, 3) for k, o in enumerate(offs)]
    vec[0] = (0, 0, 0)                                          # no such key: the first record,
    vec[4] = (offs[4], 0, 3)                                    # one in the middle (its offset and width are not looked at),
    vec[8] = (len(buf) + 100, 0, 1 << 30)
    vec[2] = (offs[2], 2, 0)                                    # a key without values,
    vec[6] = (len(buf), 3, 0)                                   # at the very end of the bytes
    want = bcfdec.decode_vec(buf, vec, S, 4)
    for k in (0, 2, 4, 6, 8):
        assert (want[k, 0] == MISSING).all() and (want[k, 1:] == VEND).all()
    with engine.Context(abi.default_cfg(S, max_sites=9, max_reads=64)) as ctx:
        np.testing.assert_array_equal(decode(ctx, buf, vec, S, 4), want)
        got = decode(ctx, b"", [(0, 0, 0), (0, 1, 0)], S, 2)    # no bytes at all
        assert (got[:, 0] == MISSING).all() and (got[:, 1] == VEND).all()


def test_no_sites():
    with engine.Context(abi.default_cfg(3, max_sites=1, max_reads=64)) as ctx:
        rc, got = call(ctx, b"\x01\x02\x03", [], 3, 15)
        assert rc == 0 and got.shape == (0, 15, 3)
        assert ctx.decode_bcf(b"", [], 3, 15).shape == (0, 15, 3)


@pytest.mark.parametrize("col", [None, "reversed"])
def test_a_run_larger_than_a_compute_units_lds(col):
    """3 records x 3000 samples x width 15 x int32: 180 000 bytes a run, more than the 160 KiB of LDS a CU has, so whatever the
    stage's size a run is taken in several slices.  A sentinel in the last sample; with a sample map every slice is a pass
    over the called samples."""
    S, w, n = 3000, 15, 3
    assert S * w * 4 > 160 * 1024
    rng = np.random.default_rng(17)
    runs = []
    for k in range(n):
        a = values(rng, S, w, 3, sentinels=0.01)
        a[S - 1, :] = rng.integers(0, 1000, w)
        a[S - 1, (0, 7, 14)[k]] = (MISSING, VEND, VEND)[k]
        runs.append(bcfdec.pack(a, 3))
    buf, offs = blocks(rng, runs, align=lambda k: (4, 9, 0)[k])
    vec = [(o, 3, w) for o in offs]
    cmap = None if col is None else np.arange(S)[::-1]
    want = bcfdec.decode_vec(buf, vec, S, w, cmap)
    last = 0 if cmap is not None else S - 1
    assert want[0, 0, last] == MISSING and want[1, 7, last] == VEND and want[2, 14, last] == VEND and want[2, 13, last] >= 0
    with engine.Context(abi.default_cfg(S, max_sites=n, max_reads=64)) as ctx:
        np.testing.assert_array_equal(decode(ctx, buf, vec, S, w, cmap), want)


def test_a_sample_as_wide_as_the_stage_and_wider():
    """Width 3840 as int32 fills the stage with one sample (a slice a sample); one value more and the samples are read from
    global memory.  Runs at an odd byte; n_planes clips both."""
    S = 3
    rng = np.random.default_rng(19)
    shape = [(3840, 3), (3841, 3), (7681, 2), (15361, 1), (15360, 1)]
    buf, offs = blocks(rng, [bcfdec.pack(values(rng, S, w, t), t) for w, t in shape], align=lambda k: (5, 3, 1, 8, 15)[k])
    vec = [(o, t, w) for o, (w, t) in zip(offs, shape)]
    with engine.Context(abi.default_cfg(S, max_sites=len(vec), max_reads=64)) as ctx:
        np.testing.assert_array_equal(decode(ctx, buf, vec, S, 15), bcfdec.decode_vec(buf, vec, S, 15))
        np.testing.assert_array_equal(decode(ctx, buf, vec, S, 15, [2, 0, 2]), bcfdec.decode_vec(buf, vec, S, 15, [2, 0, 2]))


def test_refusals_leave_the_output_alone():
    S, w = 65, 6
    rng = np.random.default_rng(23)
    buf, offs = blocks(rng, [bcfdec.pack(values(rng, S, w, 2), 2) for _ in range(3)])
    good = [(o, 2, w) for o in offs]
    end = offs[2] + S * w * 2                                   # one past the last run's last byte
    ident = list(range(S))

    def bad(k, v):
        return good[:k] + [v] + good[k + 1:]
    cases = [
        (bad(1, (offs[1], 5, w)), None, len(buf), abi.E_ARG),               # a float vector
        (bad(2, (offs[2], 4, w)), None, len(buf), abi.E_ARG),
        (bad(0, (offs[0], 2, -1)), None, len(buf), abi.E_ARG),              # a negative width
        (bad(0, (offs[0], 0, -1)), None, len(buf), abi.E_ARG),
        (good, ident[:-1] + [S], len(buf), abi.E_ARG),                      # a sample map entry equal to n_smpl_in
        (good, [-1] + ident[1:], len(buf), abi.E_ARG),
        (good, None, end - 1, abi.E_RANGE),                                 # the last run ends one byte past the bytes
        (bad(0, (end - S * w * 2 + 1, 2, w)), None, end, abi.E_RANGE),
        (bad(1, ((1 << 64) - 2, 2, w)), None, len(buf), abi.E_RANGE),       # off + bytes wraps around
    ]
    with engine.Context(abi.default_cfg(S, max_sites=3, max_reads=64)) as ctx:
        for vec, col, nbytes, code in cases:
            rc, got = call(ctx, buf, vec, S, w, col, n_indiv_bytes=nbytes)
            assert rc == code, (vec, col, nbytes, ctx.L.bcfgpu_last_error())
            assert (got.view(np.uint8) == PATTERN).all()
        with pytest.raises(engine.BcfGpuError) as e:
            ctx.decode_bcf(buf, bad(1, (offs[1], 5, w)), S, w)
        assert e.value.code == abi.E_ARG
        rc, got = call(ctx, buf, good, S, w, None, n_indiv_bytes=end)       # the exact size succeeds
        assert rc == 0
        np.testing.assert_array_equal(got, bcfdec.decode_vec(buf, good, S, w))
