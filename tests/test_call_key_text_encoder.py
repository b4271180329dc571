"""tests/helpers/keytext.py -- the twin of bcfgpu_call_parse_keys_vcf, the pass-through integer FORMAT keys of a call record of VCF text
input as BCF2 key blocks -- pinned against the text route: the host writer (host/vcfio.c, through `bcfgpu_view -O u`) and the
reference's `call` goldens.  Every integer key of every `call` input, encoded from the .vcf's own columns, is the block the writer
makes of the same file, and the twin flags none of them (the driver test's counts rest on that); the Number=R rule is checked where
the reference dropped alleles: FORMAT/AD of the golden outputs from the inputs' AD tokens and the als_map the alleles give; then known
answers against `bcfgpu_view -O u` of hand-built lines, and the values the twin flags: what the writer makes of each in the record
as it stands and in the text the driver's fallback hands it.  CPU only."""
import functools
import os
import struct

import pytest

from tests.helpers import keytext
from tests.helpers.keytext import MISSING, VEND
from tests.test_bcf_indiv_encoder import bcf_records, format_ids
from tests.test_c_host_device_call_records import CALL_ROWS
from tests.test_call_key_encoder import AD, AD_INPUTS, AD_ROWS, DP, XV, as_bcf, data_lines, declared, ints, samples_of, site_key, walk, written


@pytest.mark.parametrize("vcff", sorted({r[0] for r in CALL_ROWS}))
def test_every_integer_key_of_the_call_inputs_is_the_writers_block(golden_dir, vcff):
    path = os.path.join(golden_dir, "call", vcff)
    text, recs = bcf_records(as_bcf(path))
    ids, decl = format_ids(text), declared(text)
    lines = data_lines(path)
    S = len(samples_of(text))
    assert len(lines) == len(recs) > 0
    n = 0
    for f, (_, indiv) in zip(lines, recs):
        blocks = {b[0]: b[4] for b in walk(indiv, S)}
        nals = 1 + (0 if f[4] == "." else len(f[4].split(",")))
        for idx, name in enumerate(f[8].split(":")):
            if name in ("PL", "GT") or decl[name][1] != "Integer":
                continue
            got, status = keytext.encode_key(ids[name], f[9:], idx, nals=nals, flags=int(decl[name][0] == "R"))
            assert status == 0 and got == blocks[ids[name]], (name, f[:9])
            n += 1
    assert n > 0 or vcff in ("mpileup.vcf", "mpileup.X.vcf", "call.af-fixation.vcf", "call-G.2.vcf"), n       # (PL alone)


@functools.lru_cache(maxsize=None)
def check_ad_row(golden_dir, vcff, goldf):
    """The input record's AD tokens, als_map by matching the golden's alleles to the input's, the golden's samples as the map: the
    twin's block is the AD block of the golden's BCF form.  Returns (records compared, records that dropped an allele)."""
    G = os.path.join(golden_dir, "call")
    itext = open(os.path.join(G, vcff)).read()
    ilines = data_lines(os.path.join(G, vcff))
    gtext, grecs = bcf_records(as_bcf(os.path.join(G, goldf)))
    glines = data_lines(os.path.join(G, goldf))
    assert len(glines) == len(grecs) > 0 and declared(itext)["AD"] == ("R", "Integer")
    col = [samples_of(itext).index(x) for x in samples_of(gtext)]
    ad_out = format_ids(gtext)["AD"]
    inputs = {site_key(f): f for f in ilines}
    assert len(inputs) == len(ilines)
    dropped = compared = 0
    for g, (_, gindiv) in zip(glines, grecs):
        f = inputs[site_key(g)]
        als = [f[3]] + ([] if f[4] == "." else f[4].split(","))
        new = [g[3]] + ([] if g[4] == "." else g[4].split(","))
        als_map = [new.index(a) if a in new else -1 for a in als] + [-1] * (5 - len(als))
        want = [b for b in walk(gindiv, len(col)) if b[0] == ad_out][0][4]
        got, status = keytext.encode_key(ad_out, f[9:], f[8].split(":").index("AD"), len(als), 1, len(new), als_map, col)
        assert status == 0 and got == want, g[:9]
        compared += 1
        dropped += len(new) < len(als)
    assert compared == len(glines)
    return compared, dropped


@pytest.mark.parametrize("vcff,goldf", AD_ROWS, ids=lambda x: None)
def test_the_number_r_rule_gives_the_goldens_ad_blocks(golden_dir, vcff, goldf):
    check_ad_row(golden_dir, vcff, goldf)


def test_the_goldens_drop_alleles(golden_dir):
    got = [check_ad_row(golden_dir, v, g) for v, g in AD_ROWS]
    assert {v for v, _ in AD_ROWS} == set(AD_INPUTS) and sum(d for _, d in got) > 0 and all(c > 0 for c, _ in got)


def test_parse_token_and_output_vector():
    p, o = keytext.parse_token, keytext.output_vector
    assert p(".") == ([MISSING], True) and p("1,.,3") == ([1, MISSING, 3], True) and p("007,-0,+5") == ([7, 0, 5], True)
    assert p("-2147483648,-2147483647,2147483647") == ([MISSING, VEND, 2147483647], True)
    for bad in ("", "1,,2", "12x", " 5", "5 ", "+ 5", "2147483648", "-2147483649", "99999999999", "+", "-", "1.5", "..", "0x10"):
        assert p(bad)[1] is False, bad
    assert p("1,x,3")[0] == [1, None, 3]
    m = [0, -1, 1, -1, -1]
    assert o([1, 2, 3], True, 3, 1, 2, m) == [1, 3] and o([1, 2, 3], True, 3, 1, 1, m) == [1]
    assert o([1, 2, 3], True, 3, 0, 2, m) == [1, 2, 3] and o([1, 2, 3], True, 3, 1, 3, m) == [1, 2, 3]
    assert o([1, 2], True, 3, 1, 2, m) == [1, 2] and o([MISSING], False, 1, 1, 2, m) == [MISSING]
    assert o([7], True, 1, 1, 2, [1, -1, -1, -1, -1]) == [MISSING, 7]
    assert o([1, 2, 3], True, 3, 1, 2, [-1, 1, 1, -1, -1]) == [MISSING, 3]          # out[map[i]] = v[i] in turn: the last one stays


def test_known_answers_where_type_and_width_change():
    e = keytext.encode_key
    cols = ["10,200,3", "4,300,6"]
    # the type narrows: the only value past 127 sat on the dropped allele (G); the writer agrees on the trimmed text
    assert e(AD, cols, 0, nals=3, flags=1, nn=2, als_map=[0, -1, 1, -1, -1]) == (b"\x11\x01\x21" + bytes([10, 3, 4, 6]), 0)
    assert written("AD", ["10,3", "4,6"], alt="G")[0][4] == b"\x11\x01\x21" + bytes([10, 3, 4, 6])
    # ... and stays when the large value's allele is kept
    got = e(AD, cols, 0, nals=3, flags=1, nn=2, als_map=[0, 1, -1, -1, -1])[0]
    assert got == written("AD", ["10,200", "4,300"], alt="C")[0][4] and got[2] == 0x22
    # no allele dropped: the map is not looked at; not Number=R: neither
    assert e(AD, cols, 0, nals=3, flags=1, nn=3, als_map=[0, 2, 1, -1, -1])[0] == written("AD", cols)[0][4]
    assert e(XV, cols, 0, nals=3, flags=0, nn=2, als_map=[0, -1, 1, -1, -1])[0] == written("XV", cols)[0][4]
    # a place no kept allele fills: `missing`; one allele left: the first value alone
    assert e(AD, cols, 0, nals=3, flags=1, nn=2, als_map=[-1, -1, 1, -1, -1])[0] == written("AD", [".,3", ".,6"], alt="G")[0][4]
    assert e(AD, cols, 0, nals=3, flags=1, nn=1, als_map=[0, -1, -1, -1, -1])[0] == written("AD", ["10", "4"], alt=".")[0][4] == b"\x11\x01\x11\x0a\x04"
    # a large value on a dropped allele of a wide type: int32 in, int8 out
    assert e(AD, ["1,2000000000,3", "4,-70000,6"], 0, nals=3, flags=1, nn=2, als_map=[0, -1, 1, -1, -1])[0] == b"\x11\x01\x21" + bytes([1, 3, 4, 6])
    # '.' beside samples with a value per allele stays one value; a wrong count is left alone and widens the record
    assert e(AD, ["1,2,3", ".", "7,8,9"], 0, nals=3, flags=1, nn=2, als_map=[0, 1, -1, -1, -1])[0] == written("AD", ["1,2", ".", "7,8"], alt="C")[0][4]
    got = e(AD, ["1,2,3", "4,5", "7,8,9,10"], 0, nals=3, flags=1, nn=2, als_map=[0, -1, 1, -1, -1])[0]
    assert got == written("AD", ["1,3", "4,5", "7,8,9,10"], alt="G")[0][4] == b"\x11\x01\x41" + bytes([1, 3, 0x81, 0x81, 4, 5, 0x81, 0x81, 7, 8, 9, 10])
    # the key's place in the column, the sample map
    cols = ["1,2,3:6", "4,5,6:300", "7,8,9:24"]
    assert e(DP, cols, 1, col=[2, 0])[0] == b"\x11\x02\x11" + bytes([24, 6])
    assert e(DP, cols, 1, col=[1, 1, 0])[0] == b"\x11\x02\x12" + struct.pack("<3h", 300, 300, 6)
    assert e(AD, cols, 0, nals=3, flags=1, nn=2, als_map=[0, 1, -1, -1, -1], col=[2])[0] == b"\x11\x01\x21" + bytes([7, 8])
    assert e(DP, cols, 1)[0] == written("AD:DP", cols)[1][4]
    # the bounds of the types, a `missing` inside a vector
    for v, t in ((127, 1), (128, 2), (-120, 1), (-121, 2), (32767, 2), (32768, 3), (-32760, 2), (-32761, 3), (2147483647, 3), (-2147483646, 3)):
        got = e(XV, ["%d,.,5" % v, "0"], 0)[0]
        assert got == written("XV", ["%d,.,5" % v, "0"])[0][4] and got[2] == 0x30 | t, v


@pytest.mark.parametrize("width", [14, 15, 130])
def test_the_short_and_the_long_descriptor(width):
    cols = [",".join(str((s * 7 + j) % 100) for j in range(width)) for s in range(2)]
    got, status = keytext.encode_key(XV, cols, 0)
    assert status == 0 and got == written("XV", cols)[0][4]
    desc = {14: b"\xe1", 15: b"\xf1\x11\x0f", 130: b"\xf1\x12\x82\x00"}[width]
    assert got[:2 + len(desc)] == b"\x11\x03" + desc


def test_the_widest_key_and_the_one_past_it():
    cols = [",".join("1" for _ in range(255)), "2"]
    got, status = keytext.encode_key(XV, cols, 0)
    assert status == 0 and got == written("XV", cols)[0][4] and got[:6] == b"\x11\x03\xf1\x12\xff\x00"
    assert keytext.encode_key(XV, [",".join("1" for _ in range(256)), "2"], 0) == (b"", 2)
    # the width is the called samples': a sample map that leaves the wide column out leaves the flag out
    assert keytext.encode_key(XV, [",".join("1" for _ in range(256)), "2"], 0, col=[1]) == (b"\x11\x03\x11\x02", 0)


def test_missing_tokens_sentinel_texts_and_signs():
    e = keytext.encode_key
    # every sample '.': int8, one value; a column shorter than idx and a whole-column '.' are '.' too
    assert e(DP, [".", ".", "."], 0) == (b"\x11\x02\x11\x80\x80\x80", 0) and written("DP", [".", ".", "."])[0][4] == b"\x11\x02\x11\x80\x80\x80"
    cols = ["1,2,3:5", "4,5,6", "."]
    assert e(DP, cols, 1)[0] == written("AD:DP", cols)[1][4] == b"\x11\x02\x11\x05\x80\x80"
    # ... and an absent R token is not remapped, whatever the allele count ('.' is one value: at nals 1 a present '.' is)
    assert e(DP, ["7:."], 1, nals=1, flags=1, nn=2, als_map=[1, -1, -1, -1, -1])[0] == b"\x11\x02\x21\x80\x80"
    assert e(DP, ["7"], 1, nals=1, flags=1, nn=2, als_map=[1, -1, -1, -1, -1])[0] == b"\x11\x02\x11\x80"
    # the decimal text of the two sentinels, in the middle of a vector: stored as it stands, the vector neither cut nor shortened
    cols = ["1,-2147483648,3", "4,-2147483647,6"]
    got = e(XV, cols, 0)[0]
    assert got == written("XV", cols)[0][4] == b"\x11\x03\x31" + bytes([1, 0x80, 3, 4, 0x81, 6])
    cols = ["1,-2147483648,300", "4,-2147483647,70000"]
    assert e(XV, cols, 0)[0] == written("XV", cols)[0][4] == b"\x11\x03\x33" + ints(3, 1, MISSING, 300, 4, VEND, 70000)
    # leading zeros and signs
    cols = ["007,-0,+5", "-007,+0,0128"]
    assert e(XV, cols, 0)[0] == written("XV", cols)[0][4] == b"\x11\x03\x32" + struct.pack("<6h", 7, 0, 5, -7, 0, 128)


def fallback_text(fmt, cols, name, nals, nn, als_map, r_keys=("AD",)):
    """What the driver hands the writer for a key left to the host: the key alone in a FORMAT column of its own, every column its token
    of that key ('.' when the column has none), a Number=R token of a record that lost alleles in the alleles' new order."""
    idx, out = fmt.split(":").index(name), []
    for c in cols:
        toks = c.split(":")
        tok = toks[idx] if idx < len(toks) else "."
        v = tok.split(",")
        if idx < len(toks) and name in r_keys and nn != nals and len(v) == nals:
            o = ["."] * nn
            for i in range(nals):
                if als_map[i] >= 0:
                    o[als_map[i]] = v[i]
            tok = v[0] if nn == 1 else ",".join(o)
        out.append(tok)
    return name, out


@pytest.mark.parametrize("bad,strict,same", [("", "0", True), ("12x", "12", True), (" 5", "5", True), ("2147483648", None, False),
                                            ("-2147483649", None, False)], ids=["empty", "12x", "blank", "past-int32", "below-int32"])
def test_flagged_values_go_to_the_writer_as_the_text_route_has_them(bad, strict, same):
    """Status 1, and why: the text route hands the value to strtol, which makes a number of each.  The writer's block for the key in
    the record as it stands equals its block for the text the driver's fallback hands it (the flag changes no byte); against the
    exact reading the flag is harmless where strtol's number is the one the digits spell, and needed where it is not."""
    fmt, cols = "AD:DP", ["1,2,3:%s" % bad, "4,5,6:7"]
    assert keytext.encode_key(DP, cols, 1) == (b"", 1)
    assert keytext.encode_key(AD, cols, 0, nals=3, flags=1, nn=2, als_map=[0, -1, 1, -1, -1])[1] == 0      # the key beside it is not flagged
    in_record = written(fmt, cols)[1][4]
    name, toks = fallback_text(fmt, cols, "DP", 3, 2, [0, -1, 1, -1, -1])
    assert written(name, toks)[0][4] == in_record
    if same:                                                    # harmless: the exact grammar would have had to guess what strtol does
        assert in_record == written("DP", [strict, "7"])[0][4]
    else:                                                       # needed: strtol's value wrapped into int32 is no reading of the digits
        wrapped = (int(bad) + 2 ** 31) % 2 ** 32 - 2 ** 31
        assert in_record == keytext.encode_key(DP, ["%d" % wrapped if wrapped not in (MISSING, VEND) else ".", "7"], 0)[0]
        assert wrapped != int(bad)
    # inside an R token of a record that lost alleles: every value is checked, on a dropped allele too
    cols = ["1,%s,3:9" % bad, "4,5,6:7"]
    assert keytext.encode_key(AD, cols, 0, nals=3, flags=1, nn=2, als_map=[0, -1, 1, -1, -1]) == (b"", 1)
    name, toks = fallback_text(fmt, cols, "AD", 3, 2, [0, -1, 1, -1, -1])
    assert toks == ["1,3", "4,6"] and written(name, toks, alt="G")[0][4] == b"\x11\x01\x21" + bytes([1, 3, 4, 6])


def test_jobs_to_blocks_offsets_and_status():
    """encode_jobs: an offset and a status per job, the emit mask, the site's nals_new and als_map, the runs inside a longer text."""
    import numpy as np
    text = b"xx\t1,2,3:300\t4,5,6:7yyy\t1,2,3:1x\t4,5,6:2"
    run = np.zeros(2, dtype=keytext.RUN_DTYPE)
    run[0], run[1] = (2, 18, 0), (23, 17, 0)
    keys = np.zeros(4, dtype=keytext.KEY_DTYPE)
    keys["site"], keys["key_id"], keys["idx"], keys["nals"], keys["flags"] = [0, 0, 1, 1], [AD, DP, AD, DP], [0, 1, 0, 1], 3, [1, 0, 1, 0]
    site = [dict(nals_new=2, als_map=[0, -1, 1, -1, -1]), dict(nals_new=3, als_map=[0, 1, 2, -1, -1])]
    a, b, c = b"\x11\x01\x21" + bytes([1, 3, 4, 6]), b"\x11\x02\x12" + struct.pack("<2h", 300, 7), b"\x11\x01\x31" + bytes([1, 2, 3, 4, 5, 6])
    data, off, status = keytext.encode_jobs(text, run, keys, 2, site, 2)
    assert bytes(data) == a + b + c and off.tolist() == [0, 7, 14, 23, 23] and status.tolist() == [0, 0, 0, 1]
    data, off, status = keytext.encode_jobs(text, run, keys, 2, site, 2, emit=[0, 1])
    assert bytes(data) == c and off.tolist() == [0, 0, 0, 9, 9] and status.tolist() == [0, 0, 0, 1]
    data, off, status = keytext.encode_jobs(text, run, keys, 2, site, 1, col=[1])
    assert bytes(data) == b"\x11\x01\x21\x04\x06" + b"\x11\x02\x11\x07" + b"\x11\x01\x31\x04\x05\x06" + b"\x11\x02\x11\x02" and status.tolist() == [0] * 4
