"""What bcfgpu_call_decode_vcf is to produce, in plain Python: one FORMAT key of VCF records' sample columns, as the text file
holds them, as the int32 planes [site][plane][called sample] of bcfgpu_call_in.  The rule is the text route's
(host/bcfgpu_call.c parse_int_list; tests/helpers/bcfdec.py planes_from_text restates it on a whole line), with the grammar of
a value stated: '.' or [+-]?[0-9]+ inside int32 -- where the host's atoi takes what it can, this refuses.

    decode_text   the rule on the bytes: runs of n_smpl_in columns, each a tab and the column's text
    pack          columns -> the bytes and the runs

Test infrastructure: the yardstick for bcfgpu_call_decode_vcf (pinned in tests/test_vcf_text_decoder.py)."""
import re

import numpy as np

MISSING, VEND = -2147483648, -2147483647
VALUE = re.compile(rb"[+-]?[0-9]+\Z")


class Malformed(ValueError):
    """What the entry refuses with BCFGPU_E_ARG: .what = "columns" (found before anything is written) or "value"."""
    def __init__(self, what, msg):
        ValueError.__init__(self, msg)
        self.what = what


class OutOfRange(ValueError):
    """BCFGPU_E_RANGE: a run passes the end of the bytes."""


def value(x):
    """One value's text -> int32."""
    if x == b".":
        return MISSING
    if not VALUE.match(x):
        raise Malformed("value", "%r is not '.' or [+-]?[0-9]+" % x)
    v = int(x)
    if not -2147483648 <= v <= 2147483647:
        raise Malformed("value", "%r is outside int32" % x)
    return v


def decode_text(buf, vec, n_smpl_in, n_planes, col=None):
    """buf: bytes or np.uint8; vec: per record (off, len, idx); col: the input column of each called sample (None: every input
    column, in order).  Returns np.int32 [len(vec), n_planes, n called samples].  Every run is checked before any is parsed."""
    raw = bytes(buf) if isinstance(buf, (bytes, bytearray)) else np.ascontiguousarray(buf, np.uint8).tobytes()
    col = list(range(n_smpl_in)) if col is None else [int(c) for c in col]
    assert all(0 <= c < n_smpl_in for c in col)
    runs = []
    for k, (off, ln, idx) in enumerate(vec):
        off, ln = int(off), int(ln)
        if off + ln > len(raw):
            raise OutOfRange("run %d passes the end of the bytes" % k)
        runs.append(raw[off:off + ln])
    for k, run in enumerate(runs):
        if run[:1] != b"\t" or run.count(b"\t") != n_smpl_in:
            raise Malformed("columns", "run %d is not %d columns, each behind a tab" % (k, n_smpl_in))
    out = np.full((len(vec), n_planes, len(col)), VEND, np.int32)
    for k, run in enumerate(runs):
        idx = int(vec[k][2])
        cols = run[1:].split(b"\t")
        for s, c in enumerate(col):
            fields = cols[c].split(b":")
            if idx < 0 or idx >= len(fields):
                out[k, 0, s] = MISSING
                continue
            for j, x in enumerate(fields[idx].split(b",")[:n_planes]):      # the values past n_planes are dropped unread
                out[k, j, s] = value(x)
    return out


def pack(columns, idx=0, gap=b""):
    """columns: per record a list of column texts (bytes), or (list, idx).  Returns (bytes, [(off, len, idx)]): the runs back to
    back, `gap` in front of each."""
    buf, vec = bytearray(), []
    for rec in columns:
        cols, i = rec if isinstance(rec, tuple) else (rec, idx)
        buf += gap
        run = b"".join(b"\t" + c for c in cols)
        vec.append((len(buf), len(run), i))
        buf += run
    return bytes(buf), vec
