"""The Python decoder of tests/helpers/vcfdec.py -- the yardstick bcfgpu_call_decode_vcf is compared with -- pinned against the
text route it is to replace: on every input VCF of the `call` goldens, decode_text on the lines' sample columns (the bytes from
the ninth tab on, back to back) gives the planes host/bcfgpu_call.c's parse gives on the whole line (bcfdec.planes_from_text),
for PL and AD, with and without a sample map; every value of these files is inside the stricter grammar; hand-made known
answers; and the malformed cases.  CPU only."""
import glob
import os
import re

import numpy as np
import pytest

from tests.helpers import bcfdec, vcfdec
from tests.helpers.vcfdec import MISSING, VEND


def records(path):
    """(number of samples, the data lines) of a VCF."""
    n_smpl, lines = None, []
    for ln in open(path):
        ln = ln.rstrip("\n")
        if ln.startswith("#CHROM"):
            n_smpl = len(ln.split("\t")) - 9
        elif ln and not ln.startswith("#"):
            lines.append(ln)
    return n_smpl, lines


def runs_of(lines, key):
    """The lines that hold the key: (text buffer, vec, the lines) -- a line's columns start at its ninth tab."""
    buf, vec, kept = bytearray(), [], []
    for ln in lines:
        f = ln.split("\t")
        keys = f[8].split(":")
        if key not in keys:
            continue
        run = ln[len("\t".join(f[:9])):].encode()
        buf += b"\n"                                            # (other bytes between the runs)
        vec.append((len(buf), len(run), keys.index(key)))
        buf += run
        kept.append(ln)
    return bytes(buf), vec, kept


def test_columns_against_the_text_route_on_every_call_input(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "call", "*.vcf")))
    assert len(files) >= 14
    seen = {"PL": 0, "AD": 0}
    for f in files:
        S, lines = records(f)
        assert S >= 1 and lines
        rev = list(range(S))[::-1]
        for ln in lines:                                        # the stricter grammar refuses no value of these files
            fld = ln.split("\t")
            keys = fld[8].split(":")
            for c in fld[9:]:
                for k, x in zip(keys, c.split(":")):
                    if k in ("PL", "AD", "QS"):
                        assert all(re.fullmatch(r"\.|-?\d+", v) for v in x.split(",")), (f, x)
        for key, n_planes in (("PL", 15), ("PL", 3), ("AD", 5)):
            buf, vec, kept = runs_of(lines, key)
            if not vec:
                continue
            seen[key] += len(vec)
            want = np.array([bcfdec.planes_from_text(ln, key, n_planes) for ln in kept])
            want_rev = np.array([bcfdec.planes_from_text(ln, key, n_planes, rev) for ln in kept])
            np.testing.assert_array_equal(vcfdec.decode_text(buf, vec, S, n_planes), want)
            np.testing.assert_array_equal(vcfdec.decode_text(buf, vec, S, n_planes, rev), want_rev)
    assert seen["PL"] > 1000 and seen["AD"] > 0


def test_known_answers():
    cols = [b"0/1:.,1,2", b"0|1:3,.,4", b"./.:5,6,.",           # '.' first, in the middle, last
            b"0/0:7", b"1/1:8,9",                               # short vectors
            b"0/1", b".",                                       # too few fields; a whole-column '.'
            b"0/1:+7,-7,007", b"0/0:2147483647,-2147483646,0",
            b"x:-2147483648,-2147483647"]                       # the sentinels' own text is stored as it stands
    buf, vec = vcfdec.pack([cols], idx=1, gap=b"abc")
    got = vcfdec.decode_text(buf, vec, len(cols), 4)
    want = np.array([[MISSING, 1, 2, VEND], [3, MISSING, 4, VEND], [5, 6, MISSING, VEND], [7, VEND, VEND, VEND], [8, 9, VEND, VEND],
                     [MISSING, VEND, VEND, VEND], [MISSING, VEND, VEND, VEND], [7, -7, 7, VEND], [2147483647, -2147483646, 0, VEND],
                     [MISSING, VEND, VEND, VEND]]).T
    np.testing.assert_array_equal(got[0], want)
    assert got.dtype == np.int32 and got.shape == (1, 4, len(cols))
    np.testing.assert_array_equal(vcfdec.decode_text(buf, vec, len(cols), 2)[0], want[:2])                  # the third values are dropped
    np.testing.assert_array_equal(vcfdec.decode_text(buf, vec, len(cols), 4, [7, 0, 7])[0], want[:, [7, 0, 7]])
    # the first field of a whole-column '.' is the '.' itself; no such key
    first = vcfdec.decode_text(buf, [(vec[0][0], vec[0][1], 0)], len(cols), 2, [6])
    none = vcfdec.decode_text(buf, [(vec[0][0], vec[0][1], -1)], len(cols), 2, [0])
    np.testing.assert_array_equal(first[0], [[MISSING], [VEND]])
    np.testing.assert_array_equal(none[0], [[MISSING], [VEND]])


def test_dropped_values_are_not_read():
    buf, vec = vcfdec.pack([[b"1,2,x", b"3"]])
    np.testing.assert_array_equal(vcfdec.decode_text(buf, vec, 2, 2)[0], [[1, 3], [2, VEND]])
    with pytest.raises(vcfdec.Malformed):
        vcfdec.decode_text(buf, vec, 2, 3)


@pytest.mark.parametrize("bad", [b"", b"1,", b",1", b"1e3", b"12345678901", b"2147483648", b"-2147483649", b"-", b"+", b"1.5", b"..", b" 1", b"0x10", b"1_0"])
def test_malformed_values(bad):
    buf, vec = vcfdec.pack([[b"0/1:1,2", b"0/1:" + bad]], idx=1)
    with pytest.raises(vcfdec.Malformed) as e:
        vcfdec.decode_text(buf, vec, 2, 3)
    assert e.value.what == "value"
    np.testing.assert_array_equal(vcfdec.decode_text(buf, vec, 2, 3, [0])[0], [[1], [2], [VEND]])           # the other column alone is fine


def test_wrong_number_of_columns():
    buf, vec = vcfdec.pack([[b"1", b"2", b"3"]])
    off, ln, idx = vec[0]
    assert vcfdec.decode_text(buf, vec, 3, 1).tolist() == [[[1, 2, 3]]]
    for n_in, v in ((4, vec), (2, vec),                         # one tab too few, one too many
                    (3, [(off + 1, ln - 1, idx)]), (2, [(off + 1, ln - 1, idx)])):          # a first byte that is no tab
        with pytest.raises(vcfdec.Malformed) as e:
            vcfdec.decode_text(buf, v, n_in, 1)
        assert e.value.what == "columns"
    with pytest.raises(vcfdec.OutOfRange):
        vcfdec.decode_text(buf, [(off, ln + 1, idx)], 3, 1)
