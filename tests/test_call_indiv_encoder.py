"""tests/helpers/callenc.py -- the numpy encoder of a call record's GT, PL and GQ that the device encoder
(bcfgpu_call_encode_bcf) is compared with -- pinned against the host writer (host/vcfio.c) on the reference's `call` goldens:
every record's per-sample bytes in the BCF form of the file are walked key by key, and the GT, PL and GQ blocks must be the
twin's encoding of the values parsed from the golden's text.  Then known answers where the layout changes: missing and haploid
genotypes beside diploid ones, an all-missing PL, the type boundaries with a sentinel elsewhere in the record, a missing GQ.
Last, host/vcfio.c vio_encode_keys (through `bcfgpu_view --key-blocks`): a record put together from its keys' blocks, each
made on its own, is the record the writer makes from the text line.  CPU only."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.helpers import callenc
from tests.helpers.callenc import MISSING, VEND
from tests.test_bcf_indiv_encoder import bcf_records, format_ids
from tests.test_c_host import VIEW_EXE, build_host

# haploid samples (X), -mg0 (2), GQ and GP (af-fixation.3), -C alleles with -i lines (cAls.3)
GOLDENS = ["mpileup.1.out", "mpileup.X.out", "mpileup.2.out", "call.af-fixation.3.out", "mpileup.cAls.3.out", "mpileup.cAls.out"]
SIZE = {1: 1, 2: 2, 3: 4, 5: 4, 7: 1}


def key_blocks(indiv, n_sample):
    """[(dictionary index, width, type, the block's bytes)] of a record's per-sample part."""
    out, p = [], 0
    while p < len(indiv):
        p0 = p
        t = indiv[p] & 15
        assert indiv[p] >> 4 == 1 and t in (1, 2, 3)
        key = int.from_bytes(indiv[p + 1:p + 1 + SIZE[t]], "little")
        p += 1 + SIZE[t]
        w, t = indiv[p] >> 4, indiv[p] & 15
        p += 1
        if w == 15:
            assert indiv[p] == 0x11
            w = indiv[p + 1]
            p += 2
        p += n_sample * w * SIZE[t]
        out.append((key, w, t, indiv[p0:p]))
    assert p == len(indiv)
    return out


def golden_records(golden_dir, goldf, extra=()):
    build_host()
    path = os.path.join(golden_dir, "call", goldf)
    bcf = subprocess.run([VIEW_EXE, "-O", "u"] + list(extra) + [path], check=True, stdout=subprocess.PIPE).stdout
    text, recs = bcf_records(bcf)
    lines = [ln.rstrip("\n") for ln in open(path) if not ln.startswith("#") and ln.strip()]
    assert len(lines) == len(recs) > 0
    return bcf, format_ids(text), lines, recs


@functools.lru_cache(maxsize=None)
def check_golden(golden_dir, goldf):
    """Every GT, PL and GQ block of the golden against the twin; returns what the golden reached."""
    _, ids, lines, recs = golden_records(golden_dir, goldf)
    by_id = {v: k for k, v in ids.items()}
    n_checked, seen = 0, set()
    for line, (_, indiv) in zip(lines, recs):
        f = line.split("\t")
        planes = callenc.text_planes(f[8], f[9:])
        blocks = key_blocks(indiv, len(f) - 9)
        assert [by_id[b[0]] for b in blocks] == f[8].split(":"), line
        if "PL" not in planes:
            seen.add("no PL")
        for key, w, t, raw in blocks:
            name = by_id[key]
            if name == "GT":
                assert callenc.encode_gt(key, planes["GT"]) == raw, line
                assert t == 1
                seen.add("GT width %d" % w)
                if w == 2 and b"\x81" in raw[3:]:
                    seen.add("GT pad")
                if 0 in raw[3:]:
                    seen.add("GT missing")
            elif name == "PL":
                assert callenc.encode_pl(key, planes["PL"], len(planes["PL"])) == raw, line
                seen.add("PL type %d" % t)
            elif name == "GQ":
                assert callenc.encode_gq(key, planes["GQ"]) == raw, line
                seen.add("GQ")
            else:
                continue
            n_checked += 1
    assert n_checked >= len(lines)
    return frozenset(seen)


@pytest.mark.parametrize("goldf", GOLDENS)
def test_twin_gives_the_writers_gt_pl_gq_blocks_on_the_goldens(golden_dir, goldf):
    check_golden(golden_dir, goldf)


def test_the_goldens_reach_the_layouts_branches(golden_dir):
    """A width-1 GT (the lone '.' of -i lines, which are also the records without PL), a width-2 GT with a haploid sample's pad, a
    missing genotype, GQ, PL as int8 and as int16."""
    seen = frozenset().union(*[check_golden(golden_dir, g) for g in GOLDENS])
    assert {"GT width 1", "GT width 2", "GT pad", "GT missing", "GQ", "PL type 1", "PL type 2", "no PL"} <= seen, seen
    assert "GT pad" in check_golden(golden_dir, "mpileup.X.out") and "GQ" in check_golden(golden_dir, "call.af-fixation.3.out")


def test_known_answers_at_the_seams():
    e = callenc
    gt = np.array([[-1, -1, 1, 0], [-1, -2, -2, 1]], np.int8)           # ./.  .  1  0/1
    assert e.encode_gt(9, gt) == b"\x11\x09\x21" + bytes([0, 0, 0, 0x81, 4, 0x81, 2, 4])
    assert e.encode_gt(9, gt[:, 1:3]) == b"\x11\x09\x11" + bytes([0, 4])   # . and 1 alone: one value a sample
    assert e.encode_gt(200, gt[:, :1]) == b"\x12\xc8\x00\x21\x00\x00"
    # every PL missing: one value a sample, int8's missing -- whether the plane says `missing` or ends at once
    pl = np.full((3, 2), VEND, np.int32); pl[0, 0] = MISSING
    assert e.encode_pl(5, pl, 3) == b"\x11\x05\x11\x80\x80"
    # the type is that of the largest value; a sentinel elsewhere in the record does not decide it
    def rec(v):
        p = np.array([[0, MISSING], [v, VEND], [3, VEND]], np.int32)
        return e.encode_pl(5, p, 3)
    assert rec(127) == b"\x11\x05\x31" + bytes([0, 127, 3, 0x80, 0x81, 0x81])
    assert rec(128) == b"\x11\x05\x32" + struct.pack("<6H", 0, 128, 3, 0x8000, 0x8001, 0x8001)
    assert rec(32767) == b"\x11\x05\x32" + struct.pack("<6H", 0, 32767, 3, 0x8000, 0x8001, 0x8001)
    assert rec(32768) == b"\x11\x05\x33" + struct.pack("<6i", 0, 32768, 3, MISSING, VEND, VEND)
    assert rec(-120)[2:3] == b"\x31" and rec(-121)[2:3] == b"\x32" and rec(-32760)[2:3] == b"\x32" and rec(-32761)[2:3] == b"\x33"
    # a haploid sample in a diploid record: padded; an all-haploid record is nals wide, not ngts
    p = np.array([[0, 10], [20, 0], [30, VEND]], np.int32)
    assert e.encode_pl(5, p, 3) == b"\x11\x05\x31" + bytes([0, 20, 30, 10, 0, 0x81])
    p[2, 0] = VEND
    assert e.encode_pl(5, p, 3) == b"\x11\x05\x21" + bytes([0, 20, 10, 0])
    pl15 = np.arange(30, dtype=np.int32).reshape(2, 15).T
    assert e.encode_pl(128, pl15, 15) == b"\x12\x80\x00\xf1\x11\x0f" + bytes(range(30))
    # GQ: missing stays missing in the type of the others
    assert e.encode_gq(7, [MISSING, 5]) == b"\x11\x07\x11\x80\x05"
    assert e.encode_gq(7, [MISSING, 128]) == b"\x11\x07\x12" + struct.pack("<2H", 0x8000, 128)
    assert e.encode_gq(7, [MISSING]) == b"\x11\x07\x11\x80"


def test_planes_to_blocks_and_offsets():
    """encode_planes: one offset per site and key; PL absent when dropped, GQ only on called variant records, the emit mask."""
    S = 2
    site = [dict(ret=2, nals_new=2, pl_dropped=0), dict(ret=1, nals_new=1, pl_dropped=1), dict(ret=2, nals_new=2, pl_dropped=0)]
    gt = np.zeros((3, 2, S), np.int8); gt[:, 1, :] = 1
    pl = np.full((3, 3, S), 7, np.int32)
    gq = np.full((3, S), 40, np.int32)
    data, off = callenc.encode_planes({"GT": 1, "PL": 2, "GQ": 3}, site, gt, pl, gq, emit=[1, 1, 0])
    g = b"\x11\x01\x21" + bytes([2, 4, 2, 4])
    b0 = g + b"\x11\x02\x31" + bytes([7] * 6) + b"\x11\x03\x11" + bytes([40, 40])
    assert bytes(data) == b0 + g
    assert off.tolist() == [0, 7, 16, len(b0), len(b0) + 7, len(b0) + 7, len(b0) + 7, len(b0) + 7, len(b0) + 7, len(b0) + 7]
    data2, off2 = callenc.encode_planes((1, 2, 3), site, gt, pl, None)
    assert bytes(data2) == g + b"\x11\x02\x31" + bytes([7] * 6) + g + g + b"\x11\x02\x31" + bytes([7] * 6)


@pytest.mark.parametrize("goldf", GOLDENS)
def test_a_record_put_together_from_key_blocks_is_the_writers_record(golden_dir, goldf):
    """vio_encode_keys, reached through `bcfgpu_view --key-blocks`: every key's block made on its own, concatenated."""
    whole, _, _, _ = golden_records(golden_dir, goldf)
    pieces, _, _, _ = golden_records(golden_dir, goldf, ["--key-blocks"])
    assert pieces == whole
