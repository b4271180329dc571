"""What bcfgpu_call_decode_bcf is to produce, in numpy: one FORMAT key's integer vectors of BCF records, as they lie in the
records' per-sample bytes, as the int32 planes [site][plane][called sample] of bcfgpu_call_in.  The rule is the text route's:
a typed integer is widened as host/vcfio.c dec_int widens it (the smallest two values of int8 and int16 are `missing` and `end
of vector`; int32 passes as it is), a sample's vector is printed up to its first `end of vector` ('.' when nothing was
printed), and host/bcfgpu_call.c parses the text back into planes filled with `end of vector` beforehand.

    decode_vec        the rule on the raw bytes
    planes_from_text  the driver's present text rule restated, on the decoded VCF line
    raw_records / indiv_keys   the records' per-sample blocks of a BCF file and where each key's values lie (over
                      tests/helpers/bcf2.py, the independent reading of the specification)

Test infrastructure: the yardstick for bcfgpu_call_decode_bcf (pinned in tests/test_bcf_indiv_decoder.py)."""
import struct

import numpy as np

from tests.helpers import bcf2

MISSING, VEND = -2147483648, -2147483647
DTYPE = {1: "<i1", 2: "<i2", 3: "<i4"}


def decode_vec(indiv, vec, n_smpl_in, n_planes, col=None):
    """indiv: bytes or np.uint8; vec: per record (off, type, width); col: the input sample of each called sample (None: every
    input sample, in order).  Returns np.int32 [len(vec), n_planes, n called samples]."""
    raw = bytes(indiv) if isinstance(indiv, (bytes, bytearray)) else np.ascontiguousarray(indiv, np.uint8).tobytes()
    col = np.arange(n_smpl_in) if col is None else np.asarray(col, np.int64)
    out = np.full((len(vec), n_planes, len(col)), VEND, np.int32)
    for k, (off, ty, width) in enumerate(vec):
        off, ty, width = int(off), int(ty), int(width)
        if ty == 0 or width == 0:
            out[k, 0, :] = MISSING
            continue
        dt = np.dtype(DTYPE[ty])
        a = np.frombuffer(raw, dt, n_smpl_in * width, off).reshape(n_smpl_in, width).astype(np.int64)
        if ty != 3:                                             # dec_int: int8 -128 / -127, int16 -32768 / -32767
            lo = -(1 << (8 * dt.itemsize - 1))
            a = np.where(a == lo, MISSING, np.where(a == lo + 1, VEND, a))
        a = a[col, :min(width, n_planes)]
        ended = np.cumsum(a == VEND, axis=1) > 0               # from the first end of vector on
        a = np.where(ended, VEND, a)
        a[:, 0] = np.where(a[:, 0] == VEND, MISSING, a[:, 0])   # nothing printed: '.'
        out[k, :a.shape[1], :] = a.T
    return out


def planes_from_text(line, key, n_planes, col=None):
    """host/bcfgpu_call.c's parse of one VCF line: np.int32 [n_planes, n called samples] of FORMAT key `key`."""
    f = line.split("\t")
    keys = f[8].split(":")
    idx = keys.index(key)
    smp = f[9:]
    col = range(len(smp)) if col is None else col
    out = np.full((n_planes, len(col)), VEND, np.int32)
    for s, c in enumerate(col):
        vals = smp[c].split(":")
        if idx < len(vals):
            for j, x in enumerate(vals[idx].split(",")[:n_planes]):
                out[j, s] = MISSING if x == "." else int(x)
        else:
            out[0, s] = MISSING
    return out


def raw_records(path):
    """(bcf2.Hdr, [(indiv bytes, n_fmt, n_sample)]) of an uncompressed or BGZF-framed BCF2 file."""
    data = open(path, "rb").read()
    raw = data if data[:5] == b"BCF\x02\x02" else b"".join(r for _, r in bcf2.bgzf_blocks(data))
    l_text = struct.unpack_from("<I", raw, 5)[0]
    hdr = bcf2.Hdr(raw[9:9 + l_text].rstrip(b"\0").decode())
    off, recs = 9 + l_text, []
    while off < len(raw):
        l_shared, l_indiv = struct.unpack_from("<II", raw, off)
        nfs = struct.unpack_from("<I", raw, off + 8 + 20)[0]
        recs.append((raw[off + 8 + l_shared:off + 8 + l_shared + l_indiv], nfs >> 24, nfs & 0xffffff))
        off += 8 + l_shared + l_indiv
    return hdr, recs


def indiv_keys(hdr, ind, n_fmt, n_sample):
    """{key name: (off, type, width)} of a per-sample block: off = where value [sample 0][0] lies in the block."""
    keys, p = {}, 0
    for _ in range(n_fmt):
        n, t, p = bcf2._size(ind, p)
        (k,), p = bcf2._ints(ind, p, 1, t)
        n, t, p = bcf2._size(ind, p)
        keys[hdr.dict[k]] = (p, t, n)
        p += n * n_sample * (1 if t in (1, 7) else 2 if t == 2 else 4)
    assert p == len(ind)
    return keys


# ---- typed blocks made by hand, for the tests of the decoder ----
def pack(values, ty):
    """np array [n_smpl_in, width] of int64 holding plain values, MISSING and VEND -> the bytes of BCF2 type `ty`."""
    dt = np.dtype(DTYPE[ty])
    a = np.asarray(values, np.int64)
    if ty != 3:
        lo = -(1 << (8 * dt.itemsize - 1))
        a = np.where(a == MISSING, lo, np.where(a == VEND, lo + 1, a))
        assert a.min() >= lo and a.max() < -lo
    return a.astype(dt).tobytes()
