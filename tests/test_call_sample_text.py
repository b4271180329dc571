"""tests/helpers/callvcf.py -- the twin of bcfgpu_call_encode_vcf, the sample columns of a call record as VCF text -- pinned against
the reference's `call` goldens: for every argument row, the input record's bytes in the BCF form of the file, the als_map the
alleles give, the golden's samples as the map and the GT / PL / GQ planes parsed back from the golden line itself must give that
line's sample columns, byte for byte.  Then known answers for what no golden reaches, and the bound of include/bcfgpu.h on the
generated inputs of the GPU test.  CPU only."""
import functools
import os

import numpy as np
import pytest

from tests.helpers import callvcf
from tests.helpers.callenc import GT_MISSING, GT_VEND, MISSING, VEND, text_planes
from tests.helpers.callvcfgen import cases
from tests.test_bcf_indiv_encoder import bcf_records, format_ids
from tests.test_call_key_encoder import as_bcf, data_lines, declared, ints, samples_of, site_key, walk
from tests.test_c_host_device_call_records import CALL_ROWS

ROWS = [r for r in CALL_ROWS if r[2] != "-mg0"]


@functools.lru_cache(maxsize=None)
def check_row(golden_dir, vcff, goldf):
    """Returns (records compared, of them with an R key and an allele dropped, 1 when the golden's samples are not the input's)."""
    G = os.path.join(golden_dir, "call")
    itext, irecs = bcf_records(as_bcf(os.path.join(G, vcff)))
    ilines = data_lines(os.path.join(G, vcff))
    glines = data_lines(os.path.join(G, goldf))
    assert len(ilines) == len(irecs) and len(glines) > 0
    names, gnames = samples_of(itext), samples_of(open(os.path.join(G, goldf)).read())
    S_in, col = len(names), [names.index(x) for x in gnames]
    by_id, decl = {v: k for k, v in format_ids(itext).items()}, declared(itext)
    inputs = {site_key(f): (f, indiv) for f, (_, indiv) in zip(ilines, irecs)}
    compared = dropped_r = 0
    for g in glines:
        fmt = g[8].split(":")
        if "GP" in fmt:
            continue
        f, indiv = inputs[site_key(g)]
        als = [f[3]] + ([] if f[4] == "." else f[4].split(","))
        new = [g[3]] + ([] if g[4] == "." else g[4].split(","))
        site = dict(nals_new=len(new), als_map=[new.index(a) if a in new else -1 for a in als] + [-1] * (5 - len(als)))
        where, p = {}, 0
        for key, w, t, v0, block in walk(indiv, S_in):
            where[by_id[key]] = (p + v0, t, w)
            p += len(block)
        got = text_planes(g[8], g[9:])
        planes = {"gt": got["GT"], "pl": got.get("PL"), "gq": got.get("GQ")}
        n_gt_max = len(planes["pl"]) if planes["pl"] is not None else 1
        fields = np.zeros(len(fmt), dtype=callvcf.FIELD_DTYPE)
        has_r = False
        for i, k in enumerate(fmt):
            if k in ("GT", "PL", "GQ"):
                fields[i]["kind"] = {"GT": callvcf.GT, "PL": callvcf.PL, "GQ": callvcf.GQ}[k]
                continue
            off, t, w = where[k]
            assert t <= 3, (k, t)
            is_r = decl[k][0] == "R"
            has_r |= is_r
            fields[i] = (off, 0, callvcf.KEY, t, w, len(als), int(is_r))
        assert callvcf.site_bound(fields, n_gt_max) <= callvcf.SAMPLE_CAP
        texts = callvcf.sample_texts(planes, n_gt_max, fields, bytes(indiv), S_in, site, len(col), col)
        assert "".join(texts) == "".join("\t" + c for c in g[9:]), g[:9]
        compared += 1
        dropped_r += has_r and len(new) < len(als)
    return compared, dropped_r, int(col != list(range(S_in)))


@pytest.mark.parametrize("vcff,goldf,args", ROWS, ids=["%s:%s" % (r[1], r[2].replace("{G}/", "")) for r in ROWS])
def test_the_twin_gives_the_goldens_sample_columns(golden_dir, vcff, goldf, args):
    compared, _, _ = check_row(golden_dir, vcff, goldf)
    assert compared > 0 or "GP" in args


def test_the_goldens_drop_alleles_under_r_keys_and_use_sample_maps(golden_dir):
    got = [check_row(golden_dir, v, g) for v, g, _ in ROWS]
    assert sum(d for _, d, _ in got) > 0 and sum(m for _, _, m in got) > 0 and sum(c for c, _, _ in got) > 100


def text(fields, indiv=b"", S_in=1, nn=2, als_map=(0, 1, -1, -1, -1), gt=None, pl=None, gq=None, col=None, n_gt_max=None):
    """The sample columns of one site, through encode_fields."""
    f = np.zeros(len(fields), dtype=callvcf.FIELD_DTYPE)
    for i, x in enumerate(fields):
        f[i] = x if isinstance(x, tuple) else (0, 0, x, 0, 0, 0, 0)
    S = len(col) if col is not None else S_in
    planes = {"gt": None if gt is None else np.array([gt], np.int8), "pl": None if pl is None else np.array([pl], np.int32),
              "gq": None if gq is None else np.array([gq], np.int32)}
    data, off = callvcf.encode_fields(planes, n_gt_max or (len(pl) if pl is not None else 1), f, indiv, S_in, [dict(nals_new=nn, als_map=list(als_map))], S, col)
    assert off.tolist() == [0, len(data)]
    return data.tobytes().decode()


def key(off, t, width, nals=3, flags=0):
    return (off, 0, callvcf.KEY, t, width, nals, flags)


def test_known_answers_no_golden_reaches():
    GT, PL, GQ = callvcf.GT, callvcf.PL, callvcf.GQ
    # a negative value, '.' inside a vector, at every width of integer
    for t in (1, 2, 3):
        assert text([key(0, t, 3)], ints(t, -5, MISSING, 7, 0, VEND, VEND), S_in=2) == "\t-5,.,7\t0"
    assert text([key(0, 3, 1)], ints(3, -2147483646)) == "\t-2147483646"
    # an R key one value wider than the alleles is left alone; with a value per allele it follows them
    raw = ints(1, 1, 2, 3, 4)
    assert text([key(0, 1, 4, nals=3, flags=1)], raw, nn=2, als_map=(0, -1, 1, -1, -1)) == "\t1,2,3,4"
    assert text([key(0, 1, 3, nals=3, flags=1)], raw, nn=2, als_map=(0, -1, 1, -1, -1)) == "\t1,3"
    assert text([key(0, 1, 3, nals=3, flags=0)], raw, nn=2, als_map=(0, -1, 1, -1, -1)) == "\t1,2,3"
    assert text([key(0, 1, 3, nals=3, flags=1)], raw, nn=1, als_map=(0, -1, -1, -1, -1)) == "\t1"
    assert text([key(0, 1, 3, nals=3, flags=1)], raw, nn=2, als_map=(-1, -1, 1, -1, -1)) == "\t.,3"
    assert text([key(0, 1, 4, nals=3, flags=1)], ints(1, 1, 2, 3, VEND), nn=2, als_map=(0, 1, -1, -1, -1)) == "\t1,2"      # (padded: three values)
    # type 0 / width 0: '.'
    assert text([key(0, 0, 0), key(0, 2, 0), key(0, 0, 7)], b"", S_in=2) == "\t.:.:.\t.:.:."
    # a haploid sample in a diploid record; missing entries
    assert text([GT], S_in=3, gt=[[1, 0, GT_MISSING], [0, GT_VEND, GT_MISSING]]) == "\t1/0\t0\t./."
    # PL ending early, ending at once, missing inside, negative; only the site's ngn planes are looked at
    pl = [[10, VEND, 0], [MISSING, 5, VEND], [-3, 6, 7], [99, 99, 99]]
    assert text([PL], S_in=3, pl=pl) == "\t10,.,-3\t.\t0"
    assert text([PL], S_in=3, pl=pl, nn=1) == "\t10\t.\t0"
    assert text([PL], S_in=3, pl=pl, nn=3, n_gt_max=4) == "\t10,.,-3,99\t.\t0"
    # GQ missing
    assert text([GQ], S_in=2, gq=[MISSING, 40]) == "\t.\t40"
    # the fields in their order, the sample map on the key alone (the planes are the called samples')
    raw = ints(2, 300, 1, 2, 3, 4, 5)
    got = text([GT, key(0, 2, 2, flags=1, nals=2), PL, key(0, 2, 1), GQ], raw, S_in=3, col=[2, 0], gt=[[0, 1], [1, 1]], pl=[[0, 30], [20, 0], [40, 50]], gq=[7, MISSING])
    assert got == "\t0/1:4,5:0,20,40:2:7\t1/1:300,1:30,0,50:300:."
    # no field, no record: nothing
    assert text([]) == ""


def test_sites_offsets_and_the_emit_mask():
    f = np.zeros(3, dtype=callvcf.FIELD_DTYPE)
    f[0], f[1], f[2] = (0, 0, callvcf.GQ, 0, 0, 0, 0), (0, 2, callvcf.GQ, 0, 0, 0, 0), (0, 2, callvcf.KEY, 1, 1, 1, 0)
    site = [dict(nals_new=2, als_map=[0, 1, -1, -1, -1])] * 3
    planes = {"gq": np.array([[1, 2], [3, 4], [5, 6]], np.int32)}
    data, off = callvcf.encode_fields(planes, 1, f, ints(1, 8, 9), 2, site, 2)
    assert data.tobytes() == b"\t1\t2\t5:8\t6:9" and off.tolist() == [0, 4, 4, 12]
    data, off = callvcf.encode_fields(planes, 1, f, ints(1, 8, 9), 2, site, 2, emit=[0, 1, 1])
    assert data.tobytes() == b"\t5:8\t6:9" and off.tolist() == [0, 0, 0, 8]


@pytest.mark.parametrize("S", [1, 3, 64, 65, 257])
def test_the_bound_holds_on_the_generated_cases(S):
    """No sample's text is longer than its site's bound, and every generated site's bound is at most BCFGPU_VCF_SAMPLE_CAP: the
    entry accepts every site of the GPU test, and a round of the write kernel always takes a sample."""
    indiv, fields, site, planes, n_gt_max = cases(S)
    longest = 0
    for k in range(len(site)):
        fs = fields[fields["site"] == k]
        assert 0 < len(fs) <= callvcf.MAX_FIELDS
        bound = callvcf.site_bound(fs, n_gt_max)
        assert bound <= callvcf.SAMPLE_CAP == 15360
        here = {n: a[k] for n, a in planes.items()}
        lens = [len(t) for t in callvcf.sample_texts(here, n_gt_max, fs, bytes(indiv), S, site[k], S)]
        assert max(lens) <= bound
        longest = max(longest, max(lens))
    assert longest > 1024


def test_the_bound_formula():
    f = np.zeros(5, dtype=callvcf.FIELD_DTYPE)
    f[0]["kind"], f[1]["kind"], f[2]["kind"] = callvcf.GT, callvcf.PL, callvcf.GQ
    f[3], f[4] = key(0, 2, 3, flags=1), key(0, 0, 0)
    assert [callvcf.field_bound(x, 15) for x in f] == [4, 180, 12, 5 * 7, 5] and callvcf.site_bound(f, 15) == 1 + 4 + 180 + 12 + 35 + 5
    assert callvcf.field_bound(np.array([key(0, 1, 130)], dtype=callvcf.FIELD_DTYPE)[0], 15) == 650
    six = np.array([key(0, 3, 255)] * 6, dtype=callvcf.FIELD_DTYPE)
    assert callvcf.site_bound(six[:5], 15) == 15301 <= callvcf.SAMPLE_CAP < callvcf.site_bound(six, 15) == 18361
