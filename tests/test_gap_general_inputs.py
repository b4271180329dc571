"""The designed inputs of tests/helpers/gapgen.py against the oracle alone (no device): every scenario is valid input of
bcf_call_gap_prep -- the generator asserts the reference contract itself -- every site outside the designed dead ones is
live, and each scenario reaches the branch it was built for, shown from the oracle's results and the inputs."""
import functools

import numpy as np
import pytest

from tests.helpers import gapgen, indeldrv

SEEDS = (11, 12)
CASES = [(n, s) for n in gapgen.NAMES for s in SEEDS]


@functools.lru_cache(maxsize=None)
def oracle_runs(name, seed):
    """(batch, [per run: {site: oracle result or None}]) -- computed once, shared, never modified."""
    b = gapgen.scenario(name, seed)
    res = []
    for run in b["runs"]:
        sites = range(b["n_sites"]) if run["check"] is None else run["check"]
        res.append({k: indeldrv.gap_prep_oracle_site(b, k, **run["kw"]) for k in sites})
    return b, res


def entries(b, k):
    S = b["n_smpl"]
    return slice(int(b["smpl_off"][k * S]), int(b["smpl_off"][(k + 1) * S]))


@pytest.mark.parametrize("name,seed", CASES)
def test_designed_sites_are_live_and_dead_as_designed(name, seed):
    b, res = oracle_runs(name, seed)
    assert b["n_sites"] == len(b["pos"]) and (np.diff(b["pos"]) > 0).all()
    for run, got in zip(b["runs"], res):
        for k, w in got.items():
            assert (w is None) == (k in run["dead"]), (name, seed, run["kw"], k, int(b["pos"][k]), b["notes"][k])
        assert any(w is not None for w in got.values())
    # the pool form of the same reads: grouped by sample, position-sorted inside a sample
    smpl, rpos = b["r_smpl"], b["reads"]["r_pos"]
    assert (np.diff(smpl) >= 0).all() and ((np.diff(rpos) >= 0) | (np.diff(smpl) > 0)).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_cigars_reaches_every_path(seed):
    b, (got,) = oracle_runs("cigars", seed)
    R, ref_len = b["objs"], len(b["refseq"])
    S = b["n_smpl"]
    seen = set()
    shared = np.bincount(b["p_read"], minlength=len(R))
    assert (shared >= 2).any()                                     # reads listed in two candidate columns
    for k in range(b["n_sites"]):
        pos, sl = int(b["pos"][k]), entries(b, k)
        rd = [R[i] for i in b["p_read"][sl]]
        assert {r.l_qseq % 8 for r in rd} == set(range(8)) and min(r.l_qseq for r in rd) >= 30 and max(r.l_qseq for r in rd) <= 150
        left, right = gapgen.window(ref_len, pos, list(b["p_indel"][sl]))
        unm = sum(bool(r.flag & 4) for r in rd)
        if "type" in b["notes"][k]:
            assert 1 <= unm <= 2 and 1 <= sum(any(op == "N" for _, op in r.cigar) for r in rd)
        for r, qpos in zip(rd, b["p_qpos"][sl]):
            ops = [op for _, op in r.cigar]
            seen |= {"op" + op for op in ops}
            seen.add("lead" + ops[0])
            seen.add("trail" + ops[-1])
            n_indel = sum(op in "ID" for op in ops)
            seen.add("indels%d" % min(n_indel, 3))
            if r.flag & 4 or "N" in ops:
                continue
            if r.pos > left:
                seen.add("starts right of left")
            if r.end < right:
                seen.add("ends left of right")
            x = r.pos
            for n, op in r.cigar:
                if op == "D":
                    if x <= left < x + n:
                        seen.add("deletion over left")
                    if x <= right < x + n:
                        seen.add("deletion over right")
                    if x <= pos < x + n:
                        seen.add("in a deletion at pos")
                if op in "M=XDN":
                    x += n
    want = {"op" + c for c in "MIDNSHP=X"} | {"leadS", "leadH", "trailS", "trailH", "indels2", "indels3", "starts right of left",
                                             "ends left of right", "deletion over left", "deletion over right", "in a deletion at pos"}
    assert want <= seen, want - seen
    assert b["has_unmapped"] and not gapgen.scenario("cigars", seed, unmapped=False)["has_unmapped"]


@pytest.mark.parametrize("seed", SEEDS)
def test_repeats_reach_tandemQ_and_indelreg(seed):
    b, res = oracle_runs("repeats", seed)
    runs = [gapgen.l_run_of(b["refseq"], int(p)) for p in b["pos"]]
    assert {1, 2, 3, 4, 8, 30} <= set(runs) and sum(r >= 8 for r in runs) >= 3
    assert runs[0] == 12 and b["pos"][0] == 5                      # the run that reaches position 0
    assert b["refseq"][-7:] == b["refseq"][-1] * 7 and b["pos"][-1] == len(b["refseq"]) - 8
    assert max(w["indelreg"] for w in res[0].values()) >= 10
    assert sum(w["indelreg"] > 3 for w in res[0].values()) >= 8
    rel = set()
    for run, got in zip(b["runs"], res):
        tq = run["kw"]["tandemQ"]
        for k, w in got.items():
            for t in b["notes"][k]["types"]:
                q = 40 + 20 * (abs(t) - 1)
                qh = int(tq * abs(t) / runs[k] + .499) if runs[k] >= 3 else 1000
                rel.add("<" if q < qh else ">" if q > qh else "=")
                if runs[k] >= 3 and qh < 40:                       # tandemQ-limited: a seqQ below openQ in p->aux
                    seqq = (w["aux"] >> 8) & 0xff
                    assert ((seqq < 40) & ((w["aux"] >> 16) > 0)).any() or not ((w["aux"] >> 16) > 0).any()
    assert rel == {"<", ">", "="}
    lim = res[2][[k for k in range(b["n_sites"]) if runs[k] == 30][0]]
    alt = (lim["aux"] >> 16) > 0
    assert alt.any() and (((lim["aux"] >> 8) & 0xff)[alt] < 40).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_refletters_n_filter_and_insertion_consensus(seed):
    b, (got,) = oracle_runs("refletters", seed)
    P, so = b["keys"], b["site_of"]
    ref = b["refseq"]
    for key, nN, span in (("live100", 50, 100), ("dead101", 51, 101), ("live101", 50, 101), ("endlive", 21, 42), ("enddead", 21, 41)):
        k, p = so[P[key]], P[key]
        mx = max(b["objs"][i].l_qseq for i in b["p_read"][entries(b, k)])
        assert min(mx, len(ref) - p) == span and ref[p:p + span].count("N") == nN, key
        assert (got[k] is None) == (2 * nN > span)
    assert ref[P["N1"] + 1] == "N" and ref[P["n1"] + 1] == "n"
    win = ref[P["lower"] - 50:P["lower"] + 50]
    assert sum(c.islower() for c in win) > 40 and set("RyMk") <= set(win)
    w = got[so[P["insN"]]]
    assert list(w["indel_types"]).count(0) == 2 and w["maxins"] == 3             # the dropped insertion: type 0 twice
    w = got[so[P["tie"]]]
    assert w["maxins"] == 2 and 2 in list(w["indel_types"])
    row = list(w["indel_types"]).index(2)
    assert list(w["inscns"][2 * row:2 * row + 2]) == [0, 2]        # A and C tie 2 : 2, the first of them wins; G
    for key in ("mixins", "mixdel"):
        assert got[so[P[key]]]["indelreg"] >= 10, key


@pytest.mark.parametrize("seed", SEEDS)
def test_edges_windows_are_clipped(seed):
    b, (got,) = oracle_runs("edges", seed)
    n = len(b["refseq"])
    assert {1, 49, 50, 51} <= set(int(p) for p in b["pos"])
    ends = 0
    for k, p in enumerate(int(x) for x in b["pos"]):
        sl = entries(b, k)
        left, right = gapgen.window(n, p, list(b["p_indel"][sl]))
        assert left == (0 if p <= 50 else p - 50)
        if p > 600:
            assert right == n and p + 50 - min(b["p_indel"][sl]) > n and min(b["p_indel"][sl]) < 0
            assert p + max(b["objs"][i].l_qseq for i in b["p_read"][sl]) > n
            ends += any(b["objs"][i].end == n for i in b["p_read"][sl])
    assert ends == 3 and n - int(b["pos"][-1]) <= 4
    sl = entries(b, b["site_of"][450])                             # the longest read, 43 = 5 * 8 + 3 bases, whole inside the window
    assert max(b["objs"][i].l_qseq for i in b["p_read"][sl]) == 43 and all(400 <= b["objs"][i].pos and b["objs"][i].end <= 500 for i in b["p_read"][sl])
    assert gapgen.l_run_of(b["refseq"], 1) == 6 and gapgen.l_run_of(b["refseq"], n - 4) == 3


@pytest.mark.parametrize("seed", SEEDS)
def test_mask_columns_have_the_designed_agreement(seed):
    b, (got,) = oracle_runs("mask", seed)
    so, S = b["site_of"], b["n_smpl"]
    fr = set()
    cache = {}
    for pos, s, col, n, mm, masked in b["design"]:
        k = so[pos]
        if (k, s) not in cache:
            cache[k, s] = gapgen.column_counts(b, k, s)
        m, x = cache[k, s]
        assert (m.get(col, 0), x.get(col, 0)) == (n - mm, mm), (pos, s, col)
        if masked:
            assert (n - mm) / n < 0.7
        elif len([d for d in b["design"] if d[:2] == (pos, s)]) == 1:
            assert (n - mm) / n >= 0.7                              # (a tied column that loses to later ones is under 70 % and stays)
        fr.add((n - mm, n))
        worst = max(x.values())
        assert mm >= worst - 1                                      # no column of the window is worse than the designed ones
    assert {(7, 10), (6, 10), (13, 19)} <= fr or {(14, 20), (6, 10), (13, 19)} <= fr, fr
    empty = [k * S + s for k in range(b["n_sites"]) for s in range(S) if b["smpl_off"][k * S + s] == b["smpl_off"][k * S + s + 1]]
    assert len(empty) == b["n_sites"]                               # a sample without reads at every site


@pytest.mark.parametrize("seed", SEEDS)
def test_manytypes_counts_and_thresholds(seed):
    b, res = oracle_runs("manytypes", seed)
    P, so = b["keys"], b["site_of"]
    for nt in (5, 16, 17, 63, 64, 71):
        vals = set(int(v) for v in b["p_indel"][entries(b, so[P[nt]])])
        assert len(vals) == nt and 0 in vals and min(vals) >= -40 and max(vals) <= 30
    assert res[0][so[P[64]]] is None and res[0][so[P[63]]] is not None
    assert any(((w["aux"] >> 16) == 4).any() for w in res[0].values() if w is not None)
    sl = entries(b, so[P["on"]])
    assert (int((b["p_indel"][sl] != 0).sum()), sl.stop - sl.start) == (10, 200)
    sl = entries(b, so[P["alt9"]])
    assert (int((b["p_indel"][sl] != 0).sum()), sl.stop - sl.start) == (9, 200)
    sl = entries(b, so[P["tot205"]])
    assert (int((b["p_indel"][sl] != 0).sum()), sl.stop - sl.start) == (10, 205)
    tie = res[-1]                                                  # openQ = extQ = 0: seqQ is 0, every type's sumq is 0
    for w in tie.values():
        assert (((w["aux"] >> 8) & 0xff) == 0).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_zq_wraps_and_clamps(seed):
    b, (got,) = oracle_runs("zq", seed)
    r = b["reads"]
    S = b["n_smpl"]
    for k in range(b["n_sites"]):
        for s in range(S):
            e = slice(int(b["smpl_off"][k * S + s]), int(b["smpl_off"][k * S + s + 1]))
            assert len(set(r["r_has_zq"][b["p_read"][e]])) == 2   # mixed inside every cell
    has = np.repeat(r["r_has_zq"], r["r_lq"]).astype(bool)
    v = r["qual"][has].astype(np.int64) + r["zq"][has].astype(np.int64) - 64
    assert (v < 0).any() and ((v >= 0) & (v < 7)).any() and ((v >= 7) & (v <= 30)).any() and (v > 30).any()
    assert ((v < 0) & (v.astype(np.uint8) > 30)).any()


@pytest.mark.parametrize("seed", SEEDS)
def test_bigins_rows_past_the_output_capacity(seed):
    b, (got,) = oracle_runs("bigins", seed)
    assert sorted(w["maxins"] for w in got.values()) == [65, 70, 100, 100]
    for w in got.values():
        assert (w["indel_types"] != 10000).all() and 4 * w["maxins"] > 4 * indeldrv.CAP
        assert all(r.l_qseq == 150 for r in b["objs"])
