"""The numpy decoder of tests/helpers/bcfdec.py -- the yardstick bcfgpu_call_decode_bcf is compared with -- pinned against the
text route it is to replace: on every input VCF of the `call` goldens, turned into BCF by the host writer, decode_vec on the
raw per-sample bytes gives the planes host/bcfgpu_call.c's parse gives on the decoded line (read by the independent decoder
of tests/helpers/bcf2.py), for PL and AD; and hand-made known answers for every sentinel of every type.  CPU only."""
import glob
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import bcf2, bcfdec
from tests.helpers.bcfdec import MISSING, VEND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW = os.path.join(ROOT, "host", "bcfgpu_view")


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "bcfgpu_view"])


def test_raw_bytes_against_the_text_route_on_every_call_input(golden_dir, tmp_path):
    files = sorted(glob.glob(os.path.join(golden_dir, "call", "*.vcf")))
    assert len(files) >= 14
    seen = {"PL": 0, "AD": 0}
    types, widths = set(), set()
    for f in files:
        out = str(tmp_path / (os.path.basename(f) + ".bcf"))
        subprocess.check_call([VIEW, "-O", "u", "-o", out, f])
        _, lines = bcf2.read(out)
        hdr, recs = bcfdec.raw_records(out)
        assert len(lines) == len(recs) > 0
        S = len(hdr.samples)
        buf, offs = b"", []
        for ind, _, _ in recs:                                   # the blocks back to back, as the driver keeps them
            offs.append(len(buf))
            buf += ind
        rev = list(range(S))[::-1]
        for key, n_planes in (("PL", 15), ("PL", 3), ("AD", 5)):
            vec, want, want_rev = [], [], []
            for (ind, n_fmt, n_sample), off, line in zip(recs, offs, lines):
                assert n_sample == S
                keys = bcfdec.indiv_keys(hdr, ind, n_fmt, n_sample)
                if key not in keys:
                    continue
                o, t, w = keys[key]
                vec.append((off + o, t, w))
                types.add(t)
                widths.add(w)
                want.append(bcfdec.planes_from_text(line, key, n_planes))
                want_rev.append(bcfdec.planes_from_text(line, key, n_planes, rev))
            if not vec:
                continue
            seen[key] += len(vec)
            np.testing.assert_array_equal(bcfdec.decode_vec(buf, vec, S, n_planes), np.array(want))
            np.testing.assert_array_equal(bcfdec.decode_vec(buf, vec, S, n_planes, rev), np.array(want_rev))
    assert seen["PL"] > 1000 and seen["AD"] > 0
    assert {1, 2} <= types and {3, 6, 10} <= widths


@pytest.mark.parametrize("ty", [1, 2, 3])
def test_known_answers_for_every_sentinel(ty):
    """Five samples of width 4: a `missing` and an `end of vector` at the first, a middle and the last position."""
    hi = {1: 127, 2: 32767, 3: 2147483647}[ty]
    vals = [[MISSING, 1, 2, hi], [3, MISSING, 4, 5], [6, 7, 8, MISSING],
            [VEND, 9, 10, 11], [12, 13, VEND, 14], [15, -hi + 1, 16, VEND]]
    raw = b"\xee" * 3 + bcfdec.pack(vals, ty)                   # the run starts at byte 3
    got = bcfdec.decode_vec(raw, [(3, ty, 4)], 6, 5)[0]
    want = np.array([[MISSING, 1, 2, hi, VEND], [3, MISSING, 4, 5, VEND], [6, 7, 8, MISSING, VEND],
                     [MISSING, VEND, VEND, VEND, VEND],          # ends at once: '.'
                     [12, 13, VEND, VEND, VEND],                 # the 14 behind the end is not read
                     [15, -hi + 1, 16, VEND, VEND]]).T
    np.testing.assert_array_equal(got, want)
    clipped = bcfdec.decode_vec(raw, [(3, ty, 4)], 6, 2)[0]
    np.testing.assert_array_equal(clipped, want[:2])
    two = bcfdec.decode_vec(raw, [(3, ty, 4)], 6, 5, [4, 4])[0]
    np.testing.assert_array_equal(two, want[:, [4, 4]])


def test_known_answers_for_empty_vectors():
    all_ended = bcfdec.pack([[VEND, VEND, VEND]] * 2, 1)
    got = bcfdec.decode_vec(all_ended, [(0, 1, 3), (0, 1, 0), (0, 0, 7), (0, 2, 0)], 2, 3)
    want = np.array([[MISSING, MISSING], [VEND, VEND], [VEND, VEND]])
    for k in range(4):                                          # the all-ended vector, width 0, no such key
        np.testing.assert_array_equal(got[k], want)
    assert got.dtype == np.int32 and got.shape == (4, 3, 2)


def test_text_rule_on_dropped_trailing_fields():
    """A sample whose trailing FORMAT fields are dropped has '.' for them (the driver's `else` branch)."""
    line = "1\t1\t.\tA\tC\t.\t.\t.\tGT:PL:AD\t0/1:1,2,3:4,5\t0/0\t./.:.:.\t0/1:7,.:.,8"
    np.testing.assert_array_equal(bcfdec.planes_from_text(line, "PL", 4),
                                  np.array([[1, MISSING, MISSING, 7], [2, VEND, VEND, MISSING], [3, VEND, VEND, VEND], [VEND] * 4]))
    np.testing.assert_array_equal(bcfdec.planes_from_text(line, "AD", 2, [3, 0]), np.array([[MISSING, 4], [8, 5]]))
