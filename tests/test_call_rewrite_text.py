"""tests/helpers/callvcftext.py -- the twin of bcfgpu_call_rewrite_vcf, the sample columns of a call record rewritten from the input
record's own text -- pinned against the reference's `call` goldens: for every argument row but -mg0, the input line's sample columns,
the als_map the alleles give, the golden's samples as the map and the GT / PL / GQ planes parsed back from the golden line itself
must give that line's sample columns, byte for byte (a record that carries GP: with the GP token, which the device does not make,
taken out of the golden's columns).  Then known answers for what no golden reaches.  CPU only."""
import functools
import os

import numpy as np
import pytest

from tests.helpers import callvcftext
from tests.helpers.callenc import GT_MISSING, GT_VEND, MISSING, VEND, text_planes
from tests.helpers.callvcftextgen import cases, past_one_round, past_the_stage, STAGE
from tests.test_call_key_encoder import data_lines, declared, samples_of, site_key
from tests.test_c_host_device_call_records import CALL_ROWS

ROWS = [r for r in CALL_ROWS if r[2] != "-mg0"]


def record_of(f, decl, listed):
    """The bcfgpu_vcf_rewrite of input line f (its columns alone are the text buffer) whose written record lists the keys `listed`."""
    keys = f[8].split(":")
    rec = np.zeros(1, dtype=callvcftext.REC_DTYPE)
    text = "".join("\t" + c for c in f[9:]).encode()
    nals = 1 + (0 if f[4] == "." else len(f[4].split(",")))
    rec[0] = (0, sum(1 << i for i, k in enumerate(keys) if decl[k][0] == "R"), len(text), keys.index("PL") if "PL" in keys else -1, len(keys), nals,
              (callvcftext.FLAG_PL if "PL" in listed else 0) | (callvcftext.FLAG_GQ if "GQ" in listed else 0))
    return text, rec


@functools.lru_cache(maxsize=None)
def check_row(golden_dir, vcff, goldf):
    """Returns (records compared, of them with an R key and an allele dropped, 1 when the golden's samples are not the input's)."""
    G = os.path.join(golden_dir, "call")
    itext = open(os.path.join(G, vcff)).read()
    ilines, glines = data_lines(os.path.join(G, vcff)), data_lines(os.path.join(G, goldf))
    assert len(glines) > 0
    names, gnames = samples_of(itext), samples_of(open(os.path.join(G, goldf)).read())
    S_in, col = len(names), [names.index(x) for x in gnames]
    decl = declared(itext)
    inputs = {site_key(f): f for f in ilines}
    compared = dropped_r = 0
    for g in glines:
        fmt = g[8].split(":")
        f = inputs[site_key(g)]
        als = [f[3]] + ([] if f[4] == "." else f[4].split(","))
        new = [g[3]] + ([] if g[4] == "." else g[4].split(","))
        site = dict(nals_new=len(new), als_map=[new.index(a) if a in new else -1 for a in als] + [-1] * (5 - len(als)))
        got = text_planes(g[8], g[9:])
        planes = {"gt": got["GT"], "pl": got.get("PL"), "gq": got.get("GQ")}
        n_gt_max = len(planes["pl"]) if planes["pl"] is not None else 1
        text, rec = record_of(f, decl, fmt)
        texts = callvcftext.site_texts(planes, n_gt_max, rec[0], text, S_in, site, len(col), col)
        want = g[9:]
        if "GP" in fmt:                                             # GP is the host's: the other fields around it
            gp = fmt.index("GP")
            want = [":".join(t for i, t in enumerate(c.split(":")) if i != gp) for c in want]
        assert b"".join(texts).decode() == "".join("\t" + c for c in want), g[:9]
        compared += 1
        dropped_r += len(new) < len(als) and any(decl[k][0] == "R" for k in f[8].split(":") if k != "PL")
    return compared, dropped_r, int(col != list(range(S_in)))


@pytest.mark.parametrize("vcff,goldf,args", ROWS, ids=["%s:%s" % (r[1], r[2].replace("{G}/", "")) for r in ROWS])
def test_the_twin_gives_the_goldens_sample_columns(golden_dir, vcff, goldf, args):
    compared, _, _ = check_row(golden_dir, vcff, goldf)
    assert compared > 0


def test_the_goldens_drop_alleles_under_r_keys_and_use_sample_maps(golden_dir):
    got = [check_row(golden_dir, v, g) for v, g, _ in ROWS]
    assert len(ROWS) == 20
    assert sum(c for c, _, _ in got) > 100 and sum(d for _, d, _ in got) > 0 and sum(m for _, _, m in got) > 0


def text(cols, n_fmt, pl_idx=-1, r_mask=0, nals=3, nn=2, als_map=(0, -1, 1, -1, -1), flags=0, gt=None, pl=None, gq=None, col=None, n_gt_max=None):
    """The sample columns of one site, through rewrite()."""
    S_in = len(cols)
    S = len(col) if col is not None else S_in
    buf = b"".join(b"\t" + c for c in cols)
    rec = np.zeros(1, dtype=callvcftext.REC_DTYPE)
    rec[0] = (0, r_mask, len(buf), pl_idx, n_fmt, nals, flags)
    planes = {"gt": np.array([gt if gt is not None else [[0] * S, [1] * S]], np.int8), "pl": None if pl is None else np.array([pl], np.int32),
              "gq": None if gq is None else np.array([gq], np.int32)}
    data, off = callvcftext.rewrite(planes, n_gt_max or (len(pl) if pl is not None else 1), rec, buf, S_in, [dict(nals_new=nn, als_map=list(als_map))], S, col)
    assert off.tolist() == [0, len(data)]
    return data.tobytes()


def test_known_answers_no_golden_reaches():
    PL, GQ = callvcftext.FLAG_PL, callvcftext.FLAG_GQ
    # a column of '.' alone: the first key's token is '.', the others are absent
    assert text([b"."], 3) == b"\t0/1:.:.:."
    # fewer tokens than keys; more tokens than keys (dropped); an empty token, an empty column
    assert text([b"5:x"], 4) == b"\t0/1:5:x:.:."
    assert text([b"5:x:y:z"], 2) == b"\t0/1:5:x"
    assert text([b"5::y", b"", b":"], 3) == b"\t0/1:5::y\t0/1::.:.\t0/1:::."
    # an R field with nals values follows the alleles; with one more or one fewer it is left alone; '.' and an empty value
    assert text([b"1,2,3", b"1,2,3,4", b"1,2", b".", b"1,,3", b",,"], 1, r_mask=1) == b"\t0/1:1,3\t0/1:1,2,3,4\t0/1:1,2\t0/1:.\t0/1:1,3\t0/1:,"
    assert text([b"1,2,3"], 1, r_mask=0) == b"\t0/1:1,2,3"                               # not declared R
    assert text([b"1,2,3:4,5,6"], 2, r_mask=2) == b"\t0/1:1,2,3:4,6"                     # the second key alone
    assert text([b"1,2,3"], 1, r_mask=1, nn=3, als_map=(0, 1, 2, -1, -1)) == b"\t0/1:1,2,3"      # no allele dropped
    # nn == 1: value 0, whatever the map says
    assert text([b"7,8,9"], 1, r_mask=1, nn=1, als_map=(-1, -1, -1, -1, -1)) == b"\t0/1:7"
    # a map entry of -1 for the first allele: '.' in its place
    assert text([b"7,8,9"], 1, r_mask=1, nn=2, als_map=(-1, -1, 1, -1, -1)) == b"\t0/1:.,9"
    assert text([b"7,8,9"], 1, r_mask=1, nn=2, als_map=(1, -1, 1, -1, -1)) == b"\t0/1:.,9"       # the last one that maps there stays
    # a Float and a String token pass as the bytes they are
    assert text([b"-1.5e-07:a b,c;d=|e"], 2) == b"\t0/1:-1.5e-07:a b,c;d=|e"
    assert text([b"1.5,2.5,nan"], 1, r_mask=1) == b"\t0/1:1.5,nan"
    # PL first, last, absent; dropped (nothing, no ':'); the input's PL token is not what is written
    pl = [[10], [MISSING], [-3]]
    assert text([b"0,0,0:5"], 2, pl_idx=0, flags=PL, pl=pl, nn=2) == b"\t0/1:10,.,-3:5"
    assert text([b"5:0,0,0"], 2, pl_idx=1, flags=PL, pl=pl, nn=2) == b"\t0/1:5:10,.,-3"
    assert text([b"5"], 2, pl_idx=1, flags=PL, pl=pl, nn=2) == b"\t0/1:5:10,.,-3"         # (a column without the PL token)
    assert text([b"5:6"], 2, pl_idx=-1, pl=pl) == b"\t0/1:5:6"
    assert text([b"0,0,0:5"], 2, pl_idx=0, flags=0, pl=pl) == b"\t0/1:5"
    assert text([b"5:0,0,0"], 2, pl_idx=1, flags=0, pl=pl) == b"\t0/1:5"
    assert text([b"0,0,0"], 1, pl_idx=0, flags=0, pl=pl) == b"\t0/1"
    assert text([b"0:1"], 2, pl_idx=0, flags=PL, pl=[[VEND], [7], [7]]) == b"\t0/1:.:1"    # ends at once: '.'
    assert text([b"0:1"], 2, pl_idx=0, flags=PL, pl=pl, nn=1) == b"\t0/1:10:1"            # only the site's ngn planes
    # GT forms; GQ last, missing
    assert text([b"1", b"2", b"3"], 1, gt=[[1, 0, GT_MISSING], [0, GT_VEND, GT_MISSING]], flags=GQ, gq=[MISSING, 40, 0]) == b"\t1/0:1:.\t0:2:40\t./.:3:0"
    # the sample map picks the columns; the planes are the called samples'
    assert text([b"a", b"b", b"c"], 1, col=[2, 0, 2], gt=[[0, 1, 0], [0, 1, 1]]) == b"\t0/0:c\t1/1:a\t0/1:c"


def test_sites_offsets_and_the_emit_mask():
    buf = b"xx\t1\t2yyy\t3\t4"
    rec = np.zeros(2, dtype=callvcftext.REC_DTYPE)
    rec[0], rec[1] = (2, 0, 4, -1, 1, 1, 0), (9, 0, 4, -1, 1, 1, 0)
    site = [dict(nals_new=1, als_map=[0, -1, -1, -1, -1])] * 2
    planes = {"gt": np.array([[[0, 0], [GT_VEND, GT_VEND]]] * 2, np.int8)}
    data, off = callvcftext.rewrite(planes, 1, rec, buf, 2, site, 2)
    assert data.tobytes() == b"\t0:1\t0:2\t0:3\t0:4" and off.tolist() == [0, 8, 16]
    data, off = callvcftext.rewrite(planes, 1, rec, buf, 2, site, 2, emit=[0, 1])
    assert data.tobytes() == b"\t0:3\t0:4" and off.tolist() == [0, 0, 8]


@pytest.mark.parametrize("S", [3, 65])
def test_the_generated_cases_take_the_paths(S):
    """What tests/test_gpu_call_vcf_rewrite.py relies on: the runs start at all 16 alignments, the columns are of very unequal
    lengths, and the special shapes pass the stages where they say they do."""
    text_, rec, site, planes, ngmax = cases(S)
    assert {int(r["off"]) % 16 for r in rec} == set(range(16)) and sorted(set(int(x) for x in rec["nals"])) == [1, 2, 3, 4, 5]
    cols = [c for r in rec for c in callvcftext.columns_of(text_, r, S)]
    assert min(len(c) for c in cols) <= 1 and max(len(c) for c in cols) > 200
    assert any(int(r["flags"]) & 1 for r in rec) and any(int(r["pl_idx"]) >= 0 and not int(r["flags"]) & 1 for r in rec) and any(int(r["pl_idx"]) < 0 for r in rec)
    if S == 65:
        t, r, st, pls, g = past_one_round(S)
        out, off = callvcftext.rewrite(pls, g, r, t, S, st, S)
        assert int(r["len"][0]) > STAGE and len(out) > STAGE
        for which, n_in, n_out in (("both", True, True), ("output", False, True), ("input", True, False)):
            t, r, st, pls, g = past_the_stage(which, 3)
            c = callvcftext.columns_of(t, r[0], 3)[1]
            o = callvcftext.site_texts({k: v[0] for k, v in pls.items()}, g, r[0], t, 3, st[0], 3)[1]
            assert (1 + len(c) > STAGE) == n_in and (len(o) > STAGE) == n_out, which
