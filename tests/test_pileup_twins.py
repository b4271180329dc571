"""The two test-side pileup references against each other and against answers written out by hand (CPU only):
tests/helpers/sam.walk (a walk from the CIGAR's start for every position) and tests/helpers/cigargen.expand_read (one pass, what
follows a block from a backward pass over the operations).  Then the pools tests/test_gpu_pileup_shapes.py runs on the device:
that they reach the mechanism each is there for, and that they tell single-rule changes of the reference from the rule."""
import numpy as np
import pytest

from bcftools_amd import abi
from tests.helpers import sam, ovlfuzz, cigargen as G

# read at pos = 10; position -> (qpos, is_del, is_refskip, indel)
KNOWN = [
    ("3M2I3M", {12: (2, 0, 0, 2), 13: (5, 0, 0, 0)}),
    ("3M1P2I1P1I3M", {12: (2, 0, 0, 3), 13: (6, 0, 0, 0)}),
    ("3M2I2I3M", {12: (2, 0, 0, 4)}),
    ("3M2D3M", {12: (2, 0, 0, -2), 13: (3, 1, 0, 0), 14: (3, 1, 0, 0)}),
    ("3M1P2D3M", {12: (2, 0, 0, -2)}),
    ("3M5N3M", {12: (2, 0, 0, 0), 13: (3, 1, 1, 0), 14: (3, 1, 1, 0), 15: (3, 1, 1, 0), 16: (3, 1, 1, 0), 17: (3, 1, 1, 0)}),
    ("2S3M", {10: (2, 0, 0, 0)}),
    ("2H3M", {10: (0, 0, 0, 0)}),
    ("2I3M", {10: (2, 0, 0, 0)}),
    ("3M2I", {12: (2, 0, 0, 2)}),
    ("3M2D", {13: (3, 1, 0, 0), 14: (3, 1, 0, 0)}),
    ("2D3M", {10: (0, 1, 0, 0), 11: (0, 1, 0, 0)}),
    ("3M2I2D3M", {12: (2, 0, 0, 2), 13: (5, 1, 0, 0), 14: (5, 1, 0, 0)}),
    ("3M2D2I3M", {12: (2, 0, 0, -2), 15: (5, 0, 0, 0)}),
    ("2S2I3M1D2M3S", {10: (4, 0, 0, 0), 12: (6, 0, 0, -1), 13: (7, 1, 0, 0)}),
]


def _read(cigar, pos=10):
    return G.make_read(np.random.default_rng(0), pos, cigar)


def _expanded(r, lo=None, hi=None):
    return {t[0]: t[1:] for t in G.expand_read(r, lo, hi)}


@pytest.mark.parametrize("cigar,want", KNOWN)
def test_known_answers(cigar, want):
    r = _read(cigar)
    ex = _expanded(r)
    for pos, w in want.items():
        assert sam.walk(r, pos) == w, (cigar, pos)
        assert ex[pos] == w, (cigar, pos)
    if cigar == "3M2D":
        assert r.l_qseq == 3                      # the deletion's qpos is one past the read's last base


@pytest.mark.parametrize("cigar", ["4S", "3I"])
def test_reads_without_a_reference_span_cover_nothing(cigar):
    r = _read(cigar)
    assert _expanded(r) == {}
    assert all(sam.walk(r, p) is None for p in range(5, 20))


def _assert_twins_agree(r, positions):
    ex = _expanded(r, min(positions), max(positions) + 1)
    for p in positions:
        assert sam.walk(r, p) == ex.get(p), (getattr(r, "name", ""), r.cigar[:12], p)


def test_expand_read_agrees_with_the_walk():
    rng = np.random.default_rng(77)
    t = G.tie_reads()
    reads = G.cigar_classes() + G.long_reads() + t["same_pos"] + t["pools"][4] + [G.too_many_ops_read()]
    reads += [ovlfuzz.make_read(rng, rng.integers(0, 1000), int(rng.integers(20, 131))) for _ in range(2000)]
    n_sampled = 0
    for r in reads:
        if r.end - r.pos <= 6000:
            _assert_twins_agree(r, range(r.pos - 2, r.end + 3))
            continue
        # every operation boundary of a long read with its neighbours, and 200 positions anywhere
        pts, x = {r.pos - 2, r.pos - 1, r.end, r.end + 1, r.end + 2}, r.pos
        for l, op in r.cigar:
            if op in "M=XDN":
                pts.update((x - 1, x, x + 1, x + l - 2, x + l - 1, x + l))
                x += l
        pts.update(int(p) for p in rng.integers(r.pos, r.end, 200))
        _assert_twins_agree(r, sorted(pts))
        n_sampled += 1
    assert n_sampled == 2                          # the 65 535-base read and the 20 000-base skip


# bam2bcf.c:80-114 by hand: cigar -> {qpos: (edist, n_tot)}.  edist = qpos + 1 less every soft clip whose last base is at or before
# qpos (so the first aligned base behind a leading clip counts as 1); n_tot = M / = / X / I bases.
POSITIONS = [
    ("3S9M", {3: (1, 9), 7: (5, 9), 11: (9, 9)}),
    ("9M3S", {0: (1, 9), 4: (5, 9), 8: (9, 9)}),
    ("2S8M3S", {2: (1, 8), 5: (4, 8), 9: (8, 8)}),
    ("2H2S8M3S1H", {2: (1, 8), 5: (4, 8), 9: (8, 8)}),
    ("2S2I8M", {4: (3, 10), 7: (6, 10), 11: (10, 10)}),
    ("8M2I3S", {0: (1, 10), 3: (4, 10), 7: (8, 10)}),
    ("2S2I3M1D2M3S", {4: (3, 7), 6: (5, 7), 7: (6, 7), 8: (7, 7)}),
    ("3S4M2I4M2S", {3: (1, 10), 6: (4, 10), 12: (10, 10)}),
]


@pytest.mark.parametrize("cigar,want", POSITIONS)
def test_position_in_the_aligned_part(cigar, want):
    assert cigar in dict(G.CLASSES).values()
    r = _read(cigar)
    for qpos, (edist, n_tot) in want.items():
        assert sam.get_position(qpos, r.cigar) == (edist, n_tot)
        assert G.aligned_position(r, qpos) == (edist, n_tot)
        _, e = sam.pack_read(1, 30, 20, False, True, 0, 0, qpos, r.l_qseq, r.cigar, True)
        assert e == edist * 100 // (n_tot + 1)


# ---- the pools of the GPU cases ----
def test_case_shapes_and_sizes():
    cases = G.cases()
    for n, S in G.SHAPES:
        c = cases["shape_%dx%d" % (n, S)]
        (beg, end), = c.regions
        assert (end - beg, len(c.by_sample)) == (n, S) and beg > 0
        assert any(r.pos < beg for r in c.pool) and any(r.end > end for r in c.pool)
        if S > 2:
            assert any(not rl for rl in c.by_sample)
    items = {-(-n // 16) * -(-S // 16) for n, S in G.SHAPES}                      # workgroups with work; the grid is a multiple of 8
    assert items >= {1, 7, 8, 9, 81}
    for c in G.cases().values():
        assert all(e - b <= 64 for b, e in c.regions) or c.name in ("classes",) or c.name.startswith("shape_")
        assert len({int(q) for r in c.pool for q in r.qual}) <= 16
    assert all(e - b <= 48 for b, e in cases["long"].regions)
    assert [len(cases["pool_of_%d" % n].pool) for n in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert len(G.too_many_ops_read().cigar) == 256 and G.too_long_read().l_qseq == 65536
    assert max(len(r.cigar) for r in cases["classes"].pool) == 255 and max(r.l_qseq for r in cases["long"].pool) == 65535
    assert 190 <= len(next(r for r in cases["long"].pool if r.name == "ops200").cigar) <= 210


def test_every_class_is_seen_at_each_of_its_states():
    """In case 1's region every class shows its first and its last base, the last base of each of its blocks and every base of its
    deletions / skips."""
    c = G.cases()["classes"]
    (beg, end), = c.regions
    by_name = {r.name: r for r in c.pool}
    assert sorted(by_name) == sorted(n for n, _ in G.CLASSES) and len(c.by_sample) == 3 and len(c.by_sample[1]) == 1
    for name, cigar in G.CLASSES:
        r = by_name[name]
        ops = G.parse_cigar(cigar)
        seen = list(G.expand_read(r, beg, end))
        if not any(op in "M=XDN" for _, op in ops):
            assert seen == [] and r.end == r.pos
            continue
        assert beg < r.pos and r.end < end
        assert seen[0][0] == r.pos and seen[-1][0] == r.end - 1, name
        assert sum(1 for t in seen if t[2]) == sum(l for l, op in ops if op in "DN"), name
        assert sum(1 for t in seen if t[3]) == sum(l for l, op in ops if op == "N"), name
        # the last base of a block: the base before every place where the query offset does not go on by one
        blocks = sum(1 for _, op in ops if op in "M=X")
        x, last = r.pos, []
        for l, op in ops:
            if op in "M=XDN":
                x += l
                if op in "M=X":
                    last.append(x - 1)
        assert len(last) == blocks and all(any(t[0] == p and not t[2] for t in seen) for p in last), name
    tile, col_n, col_indel, entries = G.reference(c.name, 0)
    assert {t[2] for col in entries for t in col} >= {2, 3, 4, -1, -2}            # single, padded and doubled insertions; deletions
    # a deletion past the read's last base: base 15, quality 0 (no quality of the pools is 0)
    assert any((w >> 16) & 15 == 15 and w & 0xff == 0 and w & abi.RD_DEL for w in tile.rd.tolist())


def test_window_pool_has_the_long_skip_first_in_its_cells():
    c = G.cases()["window"]
    assert c.by_sample[0][0].cigar == [(30, "M"), (20000, "N"), (30, "M")] and len(c.by_sample[0]) == 301
    assert all(c.by_sample[0][0].pos + 30 <= r.pos < c.by_sample[0][0].end - 30 for r in c.by_sample[0][1:])
    assert len(c.by_sample[2]) == 40 and len({r.pos for r in c.by_sample[2]}) == 1 and len({r.end for r in c.by_sample[2]}) >= 30
    tile, col_n, _, entries = G.reference(c.name, 1)
    for k in range(len(col_n)):
        w = int(tile.rd[tile.plp_off[k * 3]])
        assert entries[k][0][0] == 0 and w & abi.RD_DEL and w & abi.RD_SKIP
    past, n_past, _, e_past = G.reference(c.name, 3)
    assert n_past.min() > 0 and all(t[0] != 0 for col in e_past for t in col)      # past its end: in the window, in no column


def test_three_in_order():
    c = G.cases()["three_in_order"]
    (beg, _), = c.regions
    _, _, _, entries = G.reference(c.name, 0)
    assert [sam.walk(r, 18) is not None for r in c.pool] == [False, True, True]
    assert [(t[0], sam.walk(c.pool[t[0]], 18)[1]) for t in entries[18 - beg]] == [(1, 1), (2, 0)]


def test_staging_pools_sit_on_the_capacity():
    for extra in (0, 1):
        c = G.cases()["staging_%d" % (9216 + extra)]
        tile, col_n, _, _ = G.reference(c.name, 0)
        assert len(c.by_sample) == 16                                            # one workgroup = 16 columns x 16 samples
        assert int(tile.plp_off[16 * 16]) == 9216 + extra                        # PILEUP_LDS_CAP of pileup.hip
        assert 0 < int(tile.plp_off[32 * 16] - tile.plp_off[16 * 16]) < 9216     # the next workgroup: shallow, staged


def test_alignment_pool_meets_every_start_and_length():
    c = G.cases()["alignment"]
    tile, _, _, _ = G.reference(c.name, 0)
    S = len(c.by_sample)
    assert S == 2
    b = tile.plp_off[::S].astype(np.int64)
    chunks = [(int(b[k]) & 3, int(b[k + 1] - b[k])) for k in range(32)]
    assert {(s, n & 3) for s, n in chunks} == {(s, n) for s in range(4) for n in range(4)}
    assert (1, 1) in chunks and (1, 2) in chunks                                 # shorter than the way to the next word boundary
    assert max(n for _, n in chunks) >= 8 and len(set(tile.epos.tolist())) > 20   # whole words too; bytes that differ


def test_the_walk_gives_the_same_tiles_on_every_pool():
    """On the inputs of the GPU tests the two references agree entry for entry (a disagreement of the device with them is then
    the device's)."""
    for c in G.cases().values():
        sclip = [any(op == "S" for _, op in r.cigar) for r in c.pool]
        for ri, (beg, end) in enumerate(c.regions):
            want, _, w_indel, entries = G.reference(c.name, ri)
            words, ep, off, ent = [], [], [0], []
            for pos in range(beg, end):
                k, col = 0, []
                for rl in c.by_sample:
                    for r in rl:
                        w = sam.walk(r, pos)
                        if w is not None:
                            has = w[0] < r.l_qseq
                            ww, e = sam.pack_read(sam.nt16(r.seq[w[0]]) if has else 15, int(r.qual[w[0]]) if has else 0, r.mapq, bool(r.flag & 16),
                                                  sclip[k], w[1], w[2], w[0], r.l_qseq, r.cigar, True)
                            words.append(ww); ep.append(e); col.append((k, w[0], w[3]))
                        k += 1
                    off.append(len(words))
                ent.append(col)
            np.testing.assert_array_equal(want.plp_off, np.array(off, np.uint32), err_msg=c.name)
            np.testing.assert_array_equal(want.rd, np.array(words, np.uint32), err_msg=c.name)
            np.testing.assert_array_equal(want.epos, np.array(ep, np.uint8), err_msg=c.name)
            assert entries == ent, c.name


@pytest.mark.parametrize("mut", G.MUTATIONS)
def test_pools_tell_a_changed_rule(mut):
    """Every single-rule change of the reference changes something the device is compared with (the tile's offsets, words and epos
    bytes, col_indel; on case 1's pool the entry lists too) on at least one pool the GPU tests run."""
    for c in G.cases().values():
        for ri in range(len(c.regions)):
            a, b = G.reference(c.name, ri), G.reference(c.name, ri, True, mut)
            same = (np.array_equal(a[0].plp_off, b[0].plp_off) and np.array_equal(a[0].rd, b[0].rd) and np.array_equal(a[0].epos, b[0].epos)
                    and np.array_equal(a[2], b[2]) and (a[3] == b[3] or c.name != "classes"))      # (the entry lists: case 2, on case 1's pool)
            if not same:
                return
    pytest.fail("no pool tells the rule from '%s'" % mut)


def test_without_epos_the_bytes_are_zero():
    c = G.cases()["classes"]
    a, b = G.reference(c.name, 0), G.reference(c.name, 0, False)
    assert a[0].epos.any() and not b[0].epos.any()
    np.testing.assert_array_equal(a[0].rd, b[0].rd)
