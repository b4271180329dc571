"""tests/helpers/keyenc.py -- the numpy twin of bcfgpu_call_remap_bcf, the pass-through integer FORMAT keys of a call record as BCF2
key blocks -- pinned against the host writer (host/vcfio.c) and the reference's `call` goldens.  Every integer key of every `call`
input, re-encoded from its own bytes in the BCF form of the file, is that key's block (the file came from the project's writer);
the Number=R rule is checked where the reference dropped alleles: FORMAT/AD of the golden outputs from the inputs' AD bytes and the
als_map the alleles give; then known answers where type and width change, against `bcfgpu_view -O u` of a hand-built line.
CPU only."""
import functools
import os
import re
import struct
import subprocess

import pytest

from tests.helpers import keyenc
from tests.helpers.keyenc import MISSING, VEND
from tests.test_bcf_indiv_encoder import bcf_records, format_ids
from tests.test_c_host import VIEW_EXE, build_host
from tests.test_c_host_device_call_records import CALL_ROWS

SIZE = {0: 0, 1: 1, 2: 2, 3: 4, 5: 4, 7: 1}
AD_INPUTS = ("call-G.vcf", "mpileup.hwe.vcf", "mpileup.NA19213.NA19129.vcf")


def walk(indiv, n_sample):
    """[(dictionary index, width, type, offset of the values inside the block, the block's bytes)] of a record's per-sample part."""
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
            tw = indiv[p] & 15
            assert indiv[p] >> 4 == 1 and tw in (1, 2, 3)
            w = int.from_bytes(indiv[p + 1:p + 1 + SIZE[tw]], "little")
            p += 1 + SIZE[tw]
        v0 = p
        p += n_sample * w * SIZE[t]
        out.append((key, w, t, v0 - p0, indiv[p0:p]))
    assert p == len(indiv)
    return out


def declared(text):
    """{FORMAT key: (Number, Type)} of a header."""
    return {m.group(1): (m.group(2), m.group(3)) for m in re.finditer(r"^##FORMAT=<ID=([^,]+),Number=([^,]+),Type=([^,>]+)", text, flags=re.M)}


def as_bcf(path_or_text):
    build_host()
    if os.path.exists(path_or_text):
        return subprocess.run([VIEW_EXE, "-O", "u", path_or_text], check=True, stdout=subprocess.PIPE).stdout
    return subprocess.run([VIEW_EXE, "-O", "u", "-"], input=path_or_text.encode(), check=True, stdout=subprocess.PIPE).stdout


def data_lines(path):
    return [ln.rstrip("\n").split("\t") for ln in open(path) if not ln.startswith("#") and ln.strip()]


def samples_of(text):
    return [ln for ln in text.splitlines() if ln.startswith("#CHROM")][0].split("\t")[9:]


@pytest.mark.parametrize("vcff", sorted({r[0] for r in CALL_ROWS}))
def test_every_integer_key_of_the_call_inputs_reencodes_to_itself(golden_dir, vcff):
    text, recs = bcf_records(as_bcf(os.path.join(golden_dir, "call", vcff)))
    by_id, decl = {v: k for k, v in format_ids(text).items()}, declared(text)
    S = len(samples_of(text))
    n = 0
    for _, indiv in recs:
        for key, w, t, v0, block in walk(indiv, S):
            name = by_id[key]
            if name in ("PL", "GT") or decl[name][1] != "Integer" or t > 3:
                continue
            assert keyenc.encode_key(key, block[v0:], t, w, S, nals=3, flags=decl[name][0] == "R") == block, name
            n += 1
    assert n > 0 or vcff in ("mpileup.vcf", "mpileup.X.vcf", "call.af-fixation.vcf", "call-G.2.vcf"), n       # (PL alone)


def site_key(f):
    return f[0], f[1], f[3], "INDEL" in f[7].split(";")


AD_ROWS = [(r[0], r[1]) for r in CALL_ROWS if r[0] in AD_INPUTS]


@functools.lru_cache(maxsize=None)
def check_ad_row(golden_dir, vcff, goldf):
    """The input record's AD bytes, als_map by matching the golden's alleles to the input's, the golden's samples as the map: the
    twin's block is the AD block of the golden's BCF form.  Returns (records compared, records that dropped an allele)."""
    G = os.path.join(golden_dir, "call")
    itext, irecs = bcf_records(as_bcf(os.path.join(G, vcff)))
    ilines = data_lines(os.path.join(G, vcff))
    gtext, grecs = bcf_records(as_bcf(os.path.join(G, goldf)))
    glines = data_lines(os.path.join(G, goldf))
    assert len(ilines) == len(irecs) and len(glines) == len(grecs) > 0
    assert declared(itext)["AD"] == ("R", "Integer")
    S_in, col = len(samples_of(itext)), [samples_of(itext).index(x) for x in samples_of(gtext)]
    ad_in, ad_out = format_ids(itext)["AD"], format_ids(gtext)["AD"]
    inputs = {}
    for f, (_, indiv) in zip(ilines, irecs):
        assert site_key(f) not in inputs
        inputs[site_key(f)] = (f, indiv)
    dropped = compared = 0
    for g, (_, gindiv) in zip(glines, grecs):
        f, indiv = inputs[site_key(g)]
        als = [f[3]] + ([] if f[4] == "." else f[4].split(","))
        new = [g[3]] + ([] if g[4] == "." else g[4].split(","))
        als_map = [new.index(a) if a in new else -1 for a in als] + [-1] * (5 - len(als))
        key, w, t, v0, block = [b for b in walk(indiv, S_in) if b[0] == ad_in][0]
        want = [b for b in walk(gindiv, len(col)) if b[0] == ad_out][0][4]
        assert keyenc.encode_key(ad_out, block[v0:], t, w, S_in, len(als), 1, len(new), als_map, col) == want, g[:9]
        compared += 1
        dropped += len(new) < len(als)
    assert compared == len(glines)
    return compared, dropped


@pytest.mark.parametrize("vcff,goldf", AD_ROWS, ids=lambda x: None)
def test_the_number_r_rule_gives_the_goldens_ad_blocks(golden_dir, vcff, goldf):
    check_ad_row(golden_dir, vcff, goldf)


def test_the_goldens_drop_alleles(golden_dir):
    """At least one compared record lost an allele (and so went through the remap), and every AD input was reached."""
    got = [check_ad_row(golden_dir, v, g) for v, g in AD_ROWS]
    assert {v for v, _ in AD_ROWS} == set(AD_INPUTS) and sum(d for _, d in got) > 0 and all(c > 0 for c, _ in got)


HDR = """##fileformat=VCFv4.2
##FILTER=<ID=PASS,Description="All filters passed">
##contig=<ID=1,length=1000>
##FORMAT=<ID=AD,Number=R,Type=Integer,Description="x">
##FORMAT=<ID=DP,Number=1,Type=Integer,Description="x">
##FORMAT=<ID=XV,Number=.,Type=Integer,Description="x">
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s
"""


def written(fmt, cols, alt="C,G"):
    """(per key the writer's block, the value offset inside it, width, type) of the line `1 10 . A alt . . . fmt cols...`."""
    text = HDR % "\t".join("s%d" % i for i in range(len(cols))) + "1\t10\t.\tA\t%s\t.\t.\t.\t%s\t%s\n" % (alt, fmt, "\t".join(cols))
    _, recs = bcf_records(as_bcf(text))
    assert len(recs) == 1
    return walk(recs[0][1], len(cols))


def ints(t, *vals):
    miss, vend = {1: (-128, -127), 2: (-32768, -32767), 3: (MISSING, VEND)}[t]
    return struct.pack("<%d%s" % (len(vals), " bhi"[t]), *[miss if v == MISSING else vend if v == VEND else v for v in vals])


AD, DP, XV = 1, 2, 3                                                # the dictionary indices of HDR's keys (PASS is 0)


def test_known_answers_where_type_and_width_change():
    e = keyenc.encode_key
    # the type narrows: the only value past 127 sat on the dropped allele (G); the writer agrees on the trimmed text
    raw = written("AD", ["10,200,3", "4,300,6"])[0]
    assert (raw[1], raw[2]) == (3, 2)
    got = e(AD, raw[4][raw[3]:], 2, 3, 2, nals=3, flags=1, nn=2, als_map=[0, -1, 1, -1, -1])
    assert got == b"\x11\x01\x21" + bytes([10, 3, 4, 6]) == written("AD", ["10,3", "4,6"], alt="G")[0][4]
    # ... and stays when the large value's allele is kept
    got = e(AD, raw[4][raw[3]:], 2, 3, 2, nals=3, flags=1, nn=2, als_map=[0, 1, -1, -1, -1])
    assert got == written("AD", ["10,200", "4,300"], alt="C")[0][4] and got[2] == 0x22
    # no allele dropped: the map is not looked at (the text route trims only when the allele count changes)
    assert e(AD, raw[4][raw[3]:], 2, 3, 2, nals=3, flags=1, nn=3, als_map=[0, 2, 1, -1, -1]) == raw[4]
    # a new allele order that leaves a place empty: `missing` there
    got = e(AD, raw[4][raw[3]:], 2, 3, 2, nals=3, flags=1, nn=2, als_map=[-1, -1, 1, -1, -1])
    assert got == written("AD", [".,3", ".,6"], alt="G")[0][4] == b"\x11\x01\x21" + bytes([0x80, 3, 0x80, 6])
    # nals_new 1: the first value alone
    got = e(AD, raw[4][raw[3]:], 2, 3, 2, nals=3, flags=1, nn=1, als_map=[0, -1, -1, -1, -1])
    assert got == b"\x11\x01\x11" + bytes([10, 4]) == written("AD", ["10", "4"], alt=".")[0][4]
    # the same bytes under a key that is not Number=R, or with no allele dropped: as they are
    assert e(XV, raw[4][raw[3]:], 2, 3, 2, nals=3, flags=0, nn=2, als_map=[0, -1, 1, -1, -1]) == written("XV", ["10,200,3", "4,300,6"])[0][4]
    assert e(AD, raw[4][raw[3]:], 2, 3, 2, nals=3, flags=1, nn=3, als_map=[0, 1, 2, -1, -1]) == raw[4]
    # a sample that is '.' beside samples with a value per allele: '.' stays one value, the record is nals_new wide
    raw = written("AD", ["1,2,3", ".", "7,8,9"])[0]
    got = e(AD, raw[4][raw[3]:], raw[2], raw[1], 3, nals=3, flags=1, nn=2, als_map=[0, 1, -1, -1, -1])
    assert got == b"\x11\x01\x21" + bytes([1, 2, 0x80, 0x81, 7, 8]) == written("AD", ["1,2", ".", "7,8"], alt="C")[0][4]
    # a sample with a wrong count is left alone and widens the record
    raw = written("AD", ["1,2,3", "4,5", "7,8,9,10"])[0]
    got = e(AD, raw[4][raw[3]:], raw[2], raw[1], 3, nals=3, flags=1, nn=2, als_map=[0, -1, 1, -1, -1])
    assert got == written("AD", ["1,3", "4,5", "7,8,9,10"], alt="G")[0][4]
    assert got == b"\x11\x01\x41" + bytes([1, 3, 0x81, 0x81, 4, 5, 0x81, 0x81, 7, 8, 9, 10])
    # the sample map: the second and the first sample, and one named twice
    raw = written("AD:DP", ["1,2,3:6", "4,5,6:300", "7,8,9:24"])
    assert e(DP, raw[1][4][raw[1][3]:], raw[1][2], 1, 3, col=[2, 0]) == b"\x11\x02\x11" + bytes([24, 6])
    assert e(DP, raw[1][4][raw[1][3]:], raw[1][2], 1, 3, col=[1, 1, 0]) == b"\x11\x02\x12" + struct.pack("<3h", 300, 300, 6)
    assert e(AD, raw[0][4][raw[0][3]:], 1, 3, 3, nals=3, flags=1, nn=2, als_map=[0, 1, -1, -1, -1], col=[2]) == b"\x11\x01\x21" + bytes([7, 8])


@pytest.mark.parametrize("width", [14, 15, 130])
def test_the_short_and_the_long_descriptor(width):
    cols = [",".join(str((s * 7 + j) % 100) for j in range(width)) for s in range(2)]
    key, w, t, v0, block = written("XV", cols)[0]
    assert (w, t) == (width, 1)
    assert keyenc.encode_key(XV, block[v0:], 1, width, 2) == block
    desc = {14: b"\xe1", 15: b"\xf1\x11\x0f", 130: b"\xf1\x12\x82\x00"}[width]
    assert block[:2 + len(desc)] == b"\x11\x03" + desc


def test_an_all_missing_key_and_input_that_is_not_minimal():
    e = keyenc.encode_key
    # every sample '.': int8, one value; whether the input says so in int8, in int32, with padding, or has no values at all
    want = written("DP", [".", ".", "."])[0][4]
    assert want == b"\x11\x02\x11\x80\x80\x80"
    assert e(DP, ints(1, MISSING, MISSING, MISSING), 1, 1, 3) == want
    assert e(DP, ints(3, MISSING, VEND, VEND, VEND, MISSING, VEND), 3, 2, 3) == want
    assert e(DP, b"", 0, 0, 3) == want and e(DP, b"", 2, 0, 3) == want
    # int16 holding small values; every sample padded with `end of vector`; both at once under a remap
    want = written("XV", ["1,2", "3,4"])[0][4]
    assert e(XV, ints(2, 1, 2, 3, 4), 2, 2, 2) == want
    assert e(XV, ints(1, 1, 2, VEND, VEND, 3, 4, VEND, VEND), 1, 4, 2) == want
    assert e(AD, ints(3, 1, 9, 2, VEND, 3, 9, 4, VEND), 3, 4, 2, nals=3, flags=1, nn=2, als_map=[0, -1, 1, -1, -1]) == b"\x11\x01" + want[2:]
    # a `missing` inside a vector stays, the bounds of the types
    for v, t in ((127, 1), (128, 2), (-120, 1), (-121, 2), (32767, 2), (32768, 3), (-32760, 2), (-32761, 3)):
        got = e(XV, ints(3, v, MISSING, 5, 0, VEND, VEND), 3, 3, 2)
        assert got == written("XV", ["%d,.,5" % v, "0"])[0][4] and got[2] == 0x30 | t, v


def test_jobs_to_blocks_and_offsets():
    """encode_jobs: an offset per job, the emit mask, the site's nals_new and als_map."""
    import numpy as np
    keys = np.zeros(3, dtype=keyenc.KEY_DTYPE)
    buf = ints(1, 1, 2, 3, 4, 5, 6) + ints(2, 300, 7)
    keys[0] = (0, 0, AD, 1, 3, 3, 1)
    keys[1] = (6, 0, DP, 2, 1, 3, 0)
    keys[2] = (0, 1, AD, 1, 3, 3, 1)
    site = [dict(nals_new=2, als_map=[0, -1, 1, -1, -1]), dict(nals_new=3, als_map=[0, 1, 2, -1, -1])]
    data, off = keyenc.encode_jobs(buf, keys, 2, site, 2)
    a, b, c = b"\x11\x01\x21" + bytes([1, 3, 4, 6]), b"\x11\x02\x12" + struct.pack("<2h", 300, 7), b"\x11\x01\x31" + bytes([1, 2, 3, 4, 5, 6])
    assert bytes(data) == a + b + c and off.tolist() == [0, 7, 14, 23]
    data, off = keyenc.encode_jobs(buf, keys, 2, site, 2, emit=[0, 1])
    assert bytes(data) == c and off.tolist() == [0, 0, 0, 9]
    data, off = keyenc.encode_jobs(buf, keys, 2, site, 1, col=[1])
    assert bytes(data) == b"\x11\x01\x21\x04\x06" + b"\x11\x02\x11\x07" + b"\x11\x01\x31\x04\x05\x06"
