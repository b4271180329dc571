"""Designed inputs of bcf_call_gap_prep for tests/test_gap_general_inputs.py (oracle only) and tests/test_gpu_gap_general.py:
what synth.indel_batch never makes -- general CIGARs, reads of mixed length, repeats, N / lower-case / IUPAC reference
letters, contig edges, columns under the 70 % consensus mask, many indel types, ZQ bytes, long insertions.

scenario(name, seed) places every locus by design; the seed varies bases, qualities, read placement and which reads carry
a designed mismatch.  The reads are objects (pos, cigar, bamcigar, seq, qual, flag, zq, as sam.Read / ovlfuzz.FuzzRead),
kept grouped by sample and position-sorted (stable) inside a sample: the flat pool is at once the pool of bcfgpu_pileup
and the read table of the batch, and the entries (read, qpos, indel) of every candidate column come from sam.walk in pool
order, so that bcfgpu_gap_prep and bcfgpu_pileup + bcfgpu_gap_prep_tile list them identically.  A read that spans two
candidate columns is listed in both.

Reference contract.  bcf_call_gap_prep is undefined on the inputs below (or this project's restatement of it is), so
the generator never makes them and finish() asserts each point:
  * every realigned entry (mapped, no reference skip) has qend > qbeg, the two tpos2qpos() results for the window's
    ends: the reference divides by qend - qbeg (bam2bcf_indel.c:349); the device's score 0 for "an empty side" is no contract;
  * an insertion's bases lie inside its read: p_qpos + p_indel < l_qseq (:263 reads them);
  * every entry's read covers the column (its sample then has nt >= 1 where the reference divides by nt, :135);
  * no more than 65535 reads of one sample cover a column (the consensus counters are 16 bits wide, :213);
  * seq16 holds the codes of sam.nt16 and nothing else;
  * every candidate column has ref[pos + 1] (mpileup.c:341 hands over such positions only).
Kept in, though a sanitizer build of the oracle reports them, because the reference computes the same and every compiler
in use agrees on the result: 0 / 0 in the agreement ratio of a window column that no read covers and in na / nt of a sample
without reads (NaN: the comparison fails, the column stays masked, the sample does not support), and `sc << 8` of a
realignment score of -1, which the two-base reads at the contig's start produce (an arithmetic shift).
"""
import numpy as np

from . import sam

WINDOW = 50                                   # INDEL_WINDOW_SIZE
NAMES = ("cigars", "repeats", "refletters", "edges", "mask", "manytypes", "zq", "bigins")


class GRead:
    __slots__ = ("pos", "cigar", "bamcigar", "seq", "qual", "flag", "zq", "l_qseq", "end", "mapq")


def read_base(c, x):
    """What a read shows over reference letter c at position x: the letter itself, or some base where the reference is ambiguous."""
    u = c.upper()
    return u if u in "ACGT" else "ACGT"[x & 3]


def tpos2qpos(cpos, cigar, tpos, is_left):
    """bam2bcf_indel.c:40-66 on a list of (length, op); returns (qpos, tpos)."""
    x, y, last_y = cpos, 0, 0
    for l, op in cigar:
        if op in "M=X":
            if cpos > tpos:
                return y, cpos
            if x + l > tpos:
                return y + (tpos - x), tpos
            x += l
            y += l
            last_y = y
        elif op in "IS":
            y += l
        elif op in "DN":
            if x + l > tpos:
                return y, (x if is_left else x + l)
            x += l
    return last_y, x


def window(ref_len, pos, indels):
    """left, right of bam2bcf_indel.c:173-181 for a column with these p->indel values."""
    left = pos - WINDOW if pos > WINDOW else 0
    right = pos + WINDOW - min(0, min(indels))
    return left, min(right, ref_len)


def l_run_of(ref, pos):
    """The homopolymer run around pos + 1 (bam2bcf_indel.c:236-247), ref a str."""
    n = len(ref)
    if pos + 1 >= n or sam.nt16(ref[pos + 1]) == 15:
        return 1
    c = sam.nt16(ref[pos + 1])
    i = pos + 2
    while i < n and sam.nt16(ref[i]) == c:
        i += 1
    j = pos
    while j >= 0 and sam.nt16(ref[j]) == c:
        j -= 1
    return i - (j + 1)


class Builder:
    """A contig and the reads of n_smpl samples over it.  Edit the reference first (put, run), add reads after."""

    def __init__(self, seed, n_smpl, ref_len, err=0.004):
        self.rng = np.random.default_rng(seed)
        self.S, self.err = n_smpl, err
        self.ref = ["ACGT"[i] for i in self.rng.integers(0, 4, ref_len)]
        self.by = [[] for _ in range(n_smpl)]
        self.sites = {}                       # pos -> design notes of the scenario
        self.frozen = False

    def put(self, at, s):
        assert not self.frozen and 0 <= at and at + len(s) <= len(self.ref)
        self.ref[at:at + len(s)] = list(s)

    def other(self, c, k=1):
        return "ACGT"[("ACGT".index(c.upper()) + k) & 3]

    def run(self, at, n, c):
        """A run of exactly n letters c from `at` on (the neighbours are made different)."""
        self.put(at, c * n)
        if at > 0 and self.ref[at - 1].upper() == c.upper():
            self.ref[at - 1] = self.other(c)
        if at + n < len(self.ref) and self.ref[at + n].upper() == c.upper():
            self.ref[at + n] = self.other(c, 2)

    def rand(self, n):
        return "".join("ACGT"[i] for i in self.rng.integers(0, 4, n))

    def site(self, pos, **notes):
        assert 0 <= pos and pos + 1 < len(self.ref)
        self.sites.setdefault(pos, {}).update(notes)

    def read(self, smpl, start, ops, ins=None, sub=None, flag=0, zq=None, qual=None, err=None):
        """A read from `start` with CIGAR `ops` [(length, op)]: M/=/X copy the reference (sub: {position: base} overrides),
        I takes the next bases of `ins` (random without), S is random, D/N/H/P hold no base."""
        self.frozen = True
        err = self.err if err is None else err
        x, seq, ins = start, [], list(ins or "")
        for n, op in ops:
            assert n > 0
            if op in "M=X":
                for j in range(n):
                    c = read_base(self.ref[x + j], x + j)
                    if sub and x + j in sub:
                        c = sub[x + j]
                    elif err and self.rng.random() < err:
                        c = self.other(c, int(self.rng.integers(1, 4)))
                    seq.append(c)
                x += n
            elif op == "I":
                for j in range(n):
                    seq.append(ins.pop(0) if ins else "ACGT"[int(self.rng.integers(0, 4))])
            elif op == "S":
                seq.extend(self.rand(n))
            elif op in "DN":
                x += n
        assert start >= 0 and x <= len(self.ref), (start, x, ops)
        r = GRead()
        r.pos, r.cigar, r.seq, r.flag, r.mapq = int(start), [(int(n), op) for n, op in ops], "".join(seq), flag, 60
        r.bamcigar = np.array([n << 4 | sam.CIG_OPS.index(op) for n, op in r.cigar], dtype=np.uint32)
        r.l_qseq, r.end = len(seq), x
        r.qual = self.rng.integers(8, 42, r.l_qseq).astype(np.int32) if qual is None else np.asarray(qual, np.int32)
        r.zq = zq
        assert len(r.qual) == r.l_qseq and r.l_qseq > 0
        self.by[smpl].append(r)
        return r

    def carrier(self, smpl, pos, L, off, indel=0, ins=None, **kw):
        """A read of about L bases whose base `off` sits on pos, with `indel` right after pos (aM xI/D bM, or one M)."""
        off = min(off, pos)
        i, d = max(indel, 0), max(-indel, 0)
        tail = min(L - off - 1 - i, len(self.ref) - (pos + 1) - d)
        if indel:
            assert tail >= 1, (pos, L, off, indel)
            ops = [(off + 1, "M"), (abs(indel), "I" if indel > 0 else "D"), (tail, "M")]
        else:
            ops = [(off + 1 + max(tail, 0), "M")]
        return self.read(smpl, pos - off, ops, ins=ins, **kw)

    def column(self, pos, smpl, n, carriers=(), lens=(80, 121), **kw):
        """n reads of sample smpl over pos, the first ones carrying `carriers` [(indel, count, inserted bases or None)]."""
        todo = [(ind, ins) for ind, cnt, ins in carriers for _ in range(cnt)]
        assert len(todo) <= n
        for k in range(n):
            ind, ins = todo[k] if k < len(todo) else (0, None)
            L = int(self.rng.integers(lens[0], lens[1])) + max(ind, 0)
            off = int(self.rng.integers(4, L - 5 - max(ind, 0)))
            self.carrier(smpl, pos, L, off, ind, ins, **kw)

    # ---- the batch and the pool ----
    def finish(self, name, runs=None, **design):
        for rl in self.by:
            rl.sort(key=lambda r: r.pos)                      # (stable: a position-sorted file per sample)
        pool = [r for rl in self.by for r in rl]
        r_smpl = np.array([s for s, rl in enumerate(self.by) for _ in rl], dtype=np.int32)
        first = np.concatenate([[0], np.cumsum([len(rl) for rl in self.by])])
        positions = sorted(self.sites)
        ref = "".join(self.ref)
        smpl_off, p_read, p_qpos, p_indel = [0], [], [], []
        for pos in positions:
            col0 = len(p_read)
            for s, rl in enumerate(self.by):
                assert sum(r.pos <= pos < r.end for r in rl) <= 65535
                for k, r in enumerate(rl):
                    w = sam.walk(r, pos)
                    if w is not None:
                        p_read.append(int(first[s]) + k)
                        p_qpos.append(w[0])
                        p_indel.append(w[3])
                        assert w[3] <= 0 or w[0] + w[3] < r.l_qseq, "insertion past the read's end"
                smpl_off.append(len(p_read))
            ind = p_indel[col0:]
            assert any(ind), "no indel at designed column %d" % pos
            left, right = window(len(ref), pos, ind)
            for e in range(col0, len(p_read)):                # the contract: no realignment of an empty query
                r = pool[p_read[e]]
                if r.flag & 4 or any(op == "N" for _, op in r.cigar):
                    continue
                qbeg, tbeg = tpos2qpos(r.pos, r.cigar, left, 0)
                qend, tend = tpos2qpos(r.pos, r.cigar, right, 1)
                assert qend > qbeg and left <= tbeg <= tend <= right, (name, pos, r.pos, r.cigar, qbeg, qend, tbeg, tend)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        lq, ncig = i32([r.l_qseq for r in pool]), i32([len(r.bamcigar) for r in pool])
        seq16 = np.ascontiguousarray(np.concatenate([[sam.nt16(c) for c in r.seq] for r in pool]), dtype=np.uint8)
        assert (seq16 < 16).all()
        reads = dict(n_reads=len(pool), r_pos=i32([r.pos for r in pool]), r_lq=lq, r_flag=i32([r.flag for r in pool]), r_ncig=ncig,
                     r_cig_off=i32(np.concatenate([[0], np.cumsum(ncig)[:-1]])), r_seq_off=i32(np.concatenate([[0], np.cumsum(lq)[:-1]])),
                     cig=np.ascontiguousarray(np.concatenate([r.bamcigar for r in pool]), dtype=np.uint32), seq16=seq16,
                     qual=np.ascontiguousarray(np.concatenate([r.qual for r in pool]).astype(np.uint8)),
                     zq=np.ascontiguousarray(np.concatenate([r.zq if r.zq is not None else np.zeros(r.l_qseq, np.uint8) for r in pool]), dtype=np.uint8),
                     r_has_zq=np.ascontiguousarray([r.zq is not None for r in pool], dtype=np.uint8))
        runs = runs or [dict(kw={}, dead=set(), check=None)]
        idx = {p: k for k, p in enumerate(positions)}
        return dict(name=name, ref=ref.encode(), refseq=ref, reads=reads, pos=i32(positions), smpl_off=i32(smpl_off), p_read=i32(p_read),
                    p_qpos=i32(p_qpos), p_indel=i32(p_indel), n_sites=len(positions), n_smpl=self.S, objs=pool,
                    r_mapq=np.full(len(pool), 60, np.uint8), r_smpl=r_smpl, pool=(reads, np.full(len(pool), 60, np.uint8), r_smpl, None),
                    has_unmapped=any(r.flag & 4 for r in pool), site_of=idx, notes=[self.sites[p] for p in positions],
                    runs=[dict(kw=r["kw"], dead={idx[p] for p in r["dead"]}, check=None if r["check"] is None else [idx[p] for p in r["check"]])
                          for r in runs], **design)


def column_counts(b, k, s):
    """(matches, mismatches) per reference position of sample s's entries at site k, as bam2bcf_indel.c:203-220 counts them."""
    ref, R = b["refseq"], b["objs"]
    S = b["n_smpl"]
    m, x = {}, {}
    for e in range(b["smpl_off"][k * S + s], b["smpl_off"][k * S + s + 1]):
        r = R[b["p_read"][e]]
        at, y = r.pos, 0
        for n, op in r.cigar:
            if op in "M=X":
                for j in range(n):
                    d = m if sam.nt16(r.seq[y + j]) == sam.nt16(ref[at + j]) else x
                    d[at + j] = d.get(at + j, 0) + 1
                at += n
                y += n
            elif op in "DN":
                at += n
            elif op in "IS":
                y += n
    return m, x


def host_columns(b):
    """col_n and col_indel of bcfgpu_pileup over the whole contig, from the test-side walk: the reads over every column, and
    whether some read of the column is followed by an indel."""
    n = len(b["refseq"])
    col_n, col_indel = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    for r in b["objs"]:
        col_n[r.pos:r.end] += 1
        x = r.pos
        for l, op in r.cigar:
            if op in "M=X":
                w = sam.walk(r, x + l - 1)                      # an indel follows the last base of a match block only
                col_indel[x + l - 1] |= w[3] != 0
            if op in "M=XDN":
                x += l
    return col_n, col_indel


# =====================================================================================================================
def _cigars(seed, unmapped):
    """12 sites x 4 samples x 18 reads, 16 of them of consecutive lengths (every residue mod 8) between 30 and 150."""
    n_sites, S = 12, 4
    B = Builder(seed, S, 350 + 300 * n_sites)
    rng = B.rng
    types = [-3, 2, -1, 1, -8, 4, -2, 3, -5, 1, 6, -1]
    for k in range(n_sites):
        pos, ty = 250 + 300 * k, types[k]
        left, right = window(len(B.ref), pos, [ty])
        B.site(pos, type=ty)
        made2 = False
        for s in range(S):
            base = int(rng.integers(30, 135))
            for i in range(16):
                L = base + i
                style = (i + s + k) % 16
                ind = ty if i % 3 == 0 else 0
                ii = max(ind, 0)
                flag = 0
                if style == 0:                                  # soft clips on both ends, = and X for M
                    a, c = int(rng.integers(2, 9)), int(rng.integers(1, 6))
                    body = L - a - c - ii
                    off = int(rng.integers(3, body - 3))
                    ops = [(a, "S"), (off + 1, "=")] + ([(abs(ind), "I" if ind > 0 else "D")] if ind else []) + [(body - off - 1, "X"), (c, "S")]
                    B.read(s, pos - off, ops)
                elif style == 1:                                # hard clips, a pad inside a match and one beside the indel
                    off = int(rng.integers(6, L - 8 - ii))
                    mid = [(abs(ind), "I" if ind > 0 else "D")] if ind else []
                    if ind > 0:
                        mid = [(1, "P")] + mid if k & 1 else mid + [(2, "P")]
                    ops = [(5, "H"), (3, "M"), (2, "P"), (off - 2, "M")] + mid + [(L - off - 1 - ii, "M"), (7, "H")]
                    B.read(s, pos - off, ops)
                elif style == 2 and L >= 60:                    # a second indel 12 bases right of the locus's own, a third left of it
                    off = int(rng.integers(20, L - 30 - ii))
                    ops = [(off - 9, "M"), (1, "I"), (10, "M")] + ([(abs(ind), "I" if ind > 0 else "D")] if ind else [])
                    m12 = 12 - max(-ind, 0)
                    ops += [(m12, "M"), (2, "D"), (L - off - 2 - ii - m12, "M")]
                    B.read(s, pos - off, ops)
                    made2 = True
                elif style in (3, 9) and L >= 60:               # a deletion over `left`: tbeg is its end.  (The glocal score hardly moves
                    a, D = int(rng.integers(3, 10)), int(rng.integers(25, 41))      # with the target's ends: free ends, l_ref normalised out ...
                    ops = [(a, "M"), (D, "D"), (L - a, "M")]
                    if style == 9 and L >= 90:                  # ... but the band is |l_ref - l_query| wide: this insertion needs the right tbeg)
                        ops = [(a, "M"), (D, "D"), (20, "M"), (30, "I"), (L - a - 50, "M")]
                    B.read(s, left + 5 - D - a, ops)
                elif style in (4, 10) and L >= 70:              # a deletion over `right` (tend is its start)
                    a, D = int(rng.integers(3, 10)), int(rng.integers(25, 41))
                    ops, m = [(L - a, "M"), (D, "D"), (a, "M")], L - a
                    if style == 10 and L >= 100:
                        ops, m = [(L - a - 50, "M"), (30, "I"), (20, "M"), (D, "D"), (a, "M")], L - a - 30
                    B.read(s, right - 4 - m, ops)
                elif style == 5:                                # the entry sits in a deletion at pos
                    off = int(rng.integers(8, L - 8))
                    ops = [(off - 2, "M"), (6, "D"), (L - off + 2, "M")]
                    B.read(s, pos - off, ops)
                elif style == 6:                                # a reference skip: never realigned
                    off = int(rng.integers(4, L - 9 - ii))
                    ops = [(off + 1, "M")] + ([(abs(ind), "I" if ind > 0 else "D")] if ind else []) + [(L - off - 2 - ii, "M"), (30, "N"), (1, "M")]
                    B.read(s, pos - off, ops)
                elif style == 7 and L < 90:                     # starts right of `left` and ends left of `right`: centred short read
                    off = min(L // 2, 40)
                    B.carrier(s, pos, L, off, ind)
                else:
                    if style == 8 and unmapped and s < 2:
                        flag = 4
                    off = int(rng.integers(4, L - 5 - ii))
                    B.carrier(s, pos, L, off, ind, flag=flag)
            # two more per cell, always: the straddling deletions with the insertion, whatever lengths the cell drew
            a, D, L = int(rng.integers(3, 10)), int(rng.integers(25, 41)), 104 + s
            B.read(s, left + 5 - D - a, [(a, "M"), (D, "D"), (20, "M"), (30, "I"), (L - a - 50, "M")])
            a, D, L = int(rng.integers(3, 10)), int(rng.integers(25, 41)), 112 + s
            B.read(s, right - 4 - (L - a - 30), [(L - a - 50, "M"), (30, "I"), (20, "M"), (D, "D"), (a, "M")])
        if k % 3 == 0 and made2:
            B.site(pos + 12, second=True)                       # the column of the second indel above: its reads are shared
    return B.finish("cigars")


def _repeats(seed, unmapped):
    S = 3
    B = Builder(seed, S, 5400)
    rng = B.rng
    plan = []                                                   # (pos, [(indel, inserted bases)])
    c0 = "ACGT"[seed & 3]
    B.run(0, 12, c0)                                            # a run that reaches position 0
    plan.append((5, [(-1, None), (1, c0)]))
    for k, n in enumerate((1, 2, 3, 4, 8, 30)):
        pos, c = 300 + 300 * k, "ACGT"[(seed + k) & 3]
        B.run(pos + 1, n, c)
        ty = [(-1, None), (1, c)] + ([(-4, None)] if n == 4 else [(-2, None)] if n >= 8 else [])
        plan.append((pos, ty))
        B.site(pos, run=n)
    units = ["AC", "GT", "CAG", "TTG", "AG", "CCT", "TA", "GAT"]
    reps = [5, 20, 5, 12, 9, 7, 15, 6]
    for k, (u, n) in enumerate(zip(units, reps)):
        pos = 2400 + 300 * k
        B.put(pos + 1, u * n)
        if B.ref[pos] == u[-1]:
            B.ref[pos] = B.other(u[-1])
        ty = [(-len(u), None), (len(u), u)] if k & 1 else [(-2 * len(u), None), (len(u), u), (-len(u), None)]
        plan.append((pos, ty))
        B.site(pos, unit=u, reps=n)
    last = len(B.ref) - 8                                       # a run that reaches the last base
    B.run(last + 1, 7, "ACGT"[(seed + 1) & 3])
    plan.append((last, [(-1, None)]))
    for pos, ty in plan:
        B.site(pos, types=[t for t, _ in ty])
        for s in range(S):
            B.column(pos, s, int(rng.integers(10, 15)), [(t, 2 if j == s % len(ty) else 1, ins) for j, (t, ins) in enumerate(ty)])
    return B.finish("repeats", runs=[dict(kw=dict(tandemQ=q), dead=set(), check=None) for q in (100, 30, 7)])


def _refletters(seed, unmapped):
    S = 3
    B = Builder(seed, S, 4300)
    rng = B.rng
    n = len(B.ref)
    P = {k: 300 + 300 * j for j, k in enumerate(("live100", "dead101", "N1", "n1", "lower", "mixins", "mixdel", "insN", "tie", "plain1", "plain2", "live101"))}
    P["endlive"], P["enddead"] = n - 42, n - 41               # the span is cut by the end of the contig: 42 and 41 positions
    B.put(P["live100"] + 49, "N" * 50)                          # 2 * 50 == 100: live
    B.put(P["dead101"] + 49, "N" * 51)                          # 2 * 51 == 101 + 1: dead
    B.put(P["live101"] + 49, "N" * 50)                          # the dead site's twin: 2 * 50 < 101
    B.put(n - 21, "N" * 21)                                     # 2 * 21 == 42 (live), == 41 + 1 (dead)
    B.put(P["N1"] + 1, "N")
    B.put(P["n1"] + 1, "n")
    p = P["lower"]
    B.run(p + 1, 4, "g")                                        # a lower-case run at pos + 1
    for at in range(p - 30, p + 31):
        B.ref[at] = B.ref[at].lower()
    for at, c in ((p - 22, "R"), (p - 9, "y"), (p + 14, "M"), (p + 33, "k"), (p + 40, "n")):
        B.ref[at] = c
    for key, u in (("mixins", "AC"), ("mixdel", "GTT")):       # repeats in mixed case: est_indelreg compares upper-cased letters
        p = P[key]
        B.put(p + 1, "".join(u.lower() if j & 1 else u for j in range(8)))
        if B.ref[p].upper() == u[-1]:
            B.ref[p] = B.other(u[-1])
    for key, p in P.items():
        B.site(p, key=key)
    for key, p in P.items():
        for s in range(S):
            d = int(rng.integers(10, 14))
            if key in ("live100", "dead101", "live101"):        # the longest read of the column fixes the span of the N filter
                top = 101 if key != "live100" else 100
                B.carrier(s, p, top, 10 + s, 0)
                B.column(p, s, d - 1, [(-2, 2, None)], lens=(60, 96))
            elif key in ("endlive", "enddead"):
                ty = 1 if key == "endlive" else -1
                for j in range(d // 2):
                    L = int(rng.integers(60, 100))
                    B.carrier(s, p, L, L - 30 - j, ty if j < 2 else 0, "G")
            elif key == "mixins":
                B.column(p, s, d, [(2, 2, "AC"), (-2, 1, None)])
            elif key == "mixdel":
                B.column(p, s, d, [(-3, 2, None), (3, 1, "GTT")])
            elif key == "insN":                                 # every carrier shows N at the second inserted base: the type is dropped
                B.column(p, s, d, [(3, 2, "ANC"), (-2, 2, None)])
            elif key == "tie":                                  # 2 : 2 at the first inserted base over the whole column
                ins = ["AG", "AG", "CG", "CG"] if s == 0 else []
                B.column(p, s, d, [(2, 1, x) for x in ins] + [(-1, 1, None)])
            else:
                B.column(p, s, d, [(-1 if key == "N1" else 2, 2, "TT"), (-3, 1, None)])
    return B.finish("refletters", runs=[dict(kw={}, dead={P["dead101"], P["enddead"]}, check=None)], keys=P)


def _edges(seed, unmapped):
    S = 2
    B = Builder(seed, S, 900)
    rng = B.rng
    n = len(B.ref)
    B.run(0, 6, "ACGT"[seed & 3])                               # the run scan walks off position 0 ...
    B.run(n - 3, 3, "ACGT"[(seed + 2) & 3])                     # ... and off the last base
    plan = [(1, 1), (49, -2), (50, 2), (51, -1), (300, -3), (320, 1), (600, 3), (n - 50, -10), (n - 21, -5), (n - 4, -1)]
    for pos, ty in plan:
        B.site(pos, type=ty)
        room = n - (pos + 1) - max(-ty, 0)                      # reference left for the match after the indel
        for s in range(S):
            for j in range(int(rng.integers(10, 15))):
                ind = ty if j < 3 else 0
                off = int(rng.integers(0, min(pos, 80) + 1))
                tail = room if j == 3 and room <= 100 else int(rng.integers(1, min(room, 60) + 1))     # (j == 3: ends on the last base)
                B.carrier(s, pos, off + 1 + max(ind, 0) + tail, off, ind)
    # a column whose longest read (43 bases: five 8-byte groups and a tail of 3) lies inside the window whole: its packed query
    # fills the site's stride max_rd_len rounded up to 8
    B.site(450, type=-2, short=True)
    for s in range(S):
        for j in range(12):
            L = 43 if j == 5 else int(rng.integers(33, 43))
            B.carrier(s, 450, L, L // 2 + int(rng.integers(-4, 5)), -2 if j < 3 else 0)
    return B.finish("edges")


def _mask(seed, unmapped):
    """Every read spans the whole window, no sequencing errors: the only mismatches are the designed ones."""
    S = 5
    n_sites = 10
    B = Builder(seed, S, 300 + 300 * n_sites, err=0.0)
    rng = B.rng
    design = []                                                 # (pos, sample, column, reads, mismatches, masked)
    for k in range(n_sites):
        pos = 250 + 300 * k
        ty = (-3, 2)[k & 1]
        left, right = window(len(B.ref), pos, [ty])
        B.site(pos, type=ty)
        free = [c for c in range(left + 3, right - 12) if not pos - 2 <= c <= pos + 8]
        for s in range(S):
            if s == (k + 4) % S:
                continue                                        # a sample without reads
            n = (10, 19, 20, 10, 14)[(s + k) % 5]
            x, y, z = sorted(int(c) for c in rng.choice(free, 3, replace=False))
            mode = (s + 2 * k) % 6
            M = {10: 4, 19: 6, 20: 7, 14: 5}[n]                 # the fewest mismatches under 70 % agreement: 6/10, 13/19, 13/20, 9/14
            if mode == 0:                                       # exactly 7/10 (or better): not masked
                cols, want = [(x, 3 * n // 10 if n in (10, 20) else M - 1)], [(x, False)]
            elif mode == 1:
                cols, want = [(x, M)], [(x, True)]
            elif mode == 2:                                     # two columns tied under a worse one: the last of the two
                cols, want = [(x, M), (y, M), (z, M + 1)], [(x, False), (y, True), (z, True)]
            elif mode == 3:                                     # three tied: the last two
                cols, want = [(x, M), (y, M), (z, M)], [(x, False), (y, True), (z, True)]
            elif mode == 4:                                     # the column of pos itself, and one right of the deletion's end
                r = pos + 1 + max(-ty, 0) + 2
                cols, want = [(pos, M), (r, M + 1)], [(pos, True), (r, True)]
            else:                                               # reads that stop 10 columns short of `right`
                cols, want = [(x, M)], [(x, True)]
            short = 10 if mode == 5 else 0
            who = {c: set(int(i) for i in rng.choice(np.arange(3, n), m, replace=False)) for c, m in cols}
            for j in range(n):
                sub = {c: B.other(read_base(B.ref[c], c), 1 + j % 3) for c in who if j in who[c]}
                ind = ty if j < 3 and s in (0, 1, 2) else 0
                start = left - int(rng.integers(2, 9))
                a, b2 = pos + 1 - start, right - short - (pos + 1) - max(-ind, 0)
                ops = [(a, "M"), (abs(ind), "I" if ind > 0 else "D"), (b2, "M")] if ind else [(a + b2, "M")]
                B.read(s, start, ops, sub=sub, ins="GA")
            for (c, m), (_, masked) in zip(cols, want):
                design.append((pos, s, c, n, m, masked))
    return B.finish("mask", design=design)


def _manytypes(seed, unmapped):
    S = 6
    B = Builder(seed, S, 300 + 300 * 9)
    rng = B.rng
    vals = [v for v in range(-40, 31) if v]                     # 70 distinct non-zero lengths
    P = {}
    for k, nt in enumerate((5, 16, 17, 63, 64, 71)):            # n_types, the zero type included
        pos = P[nt] = 250 + 300 * k
        B.site(pos, n_types=nt)
        if nt == 71:
            pick = list(vals)
        elif nt >= 63:                                          # (with the widest window and band the lengths allow)
            pick = [-40, 30] + list(rng.permutation([v for v in vals if v not in (-40, 30)])[:nt - 3])
        else:
            pick = list(rng.permutation(vals)[:nt - 1])
        pick = [int(v) for v in pick]
        assert len(set(pick)) == nt - 1
        depth = 40
        todo = pick + [pick[j % len(pick)] for j in range(len(pick), max(len(pick), 2 * S))]
        per = [[] for _ in range(S)]
        for j, v in enumerate(todo):
            per[j % S].append(v)
        for s in range(S):
            B.column(pos, s, max(depth, len(per[s]) + 4), [(v, 1, None) for v in per[s]], lens=(100, 121))
    # support thresholds: n_alt / n_tot and, per sample, na / nt exactly on and one below min_support and min_frac
    for key, k, na, nt in (("on", 6, (2, 2, 2, 2, 2), 40), ("alt9", 7, (2, 2, 2, 2, 1), 40), ("tot205", 8, (2, 2, 2, 2, 2), 41)):
        pos = P[key] = 250 + 300 * k
        B.site(pos, threshold=key)
        for s in range(5):                                      # (the sixth sample has no reads here)
            B.column(pos, s, nt, [(-2, na[s] - 1, None), (1, 1, "T")] if na[s] > 1 else [(-2, 1, None)], lens=(100, 121))
    thr = [P["on"], P["alt9"], P["tot205"], P[5]]
    runs = [dict(kw={}, dead={P[64], P[71]}, check=None),
            dict(kw=dict(min_support=10, min_frac=0.05), dead={P[64], P[71], P["alt9"], P["tot205"]}, check=thr),
            dict(kw=dict(min_support=2, min_frac=0.05, per_sample_flt=1), dead={P[64], P[71], P["tot205"]}, check=thr),
            dict(kw=dict(min_support=3, min_frac=0.05, per_sample_flt=1), dead={P[64], P[71], P["tot205"], P["on"], P["alt9"], P[5]}, check=thr + [P[16]]),
            dict(kw=dict(openQ=0, extQ=0), dead={P[64], P[71]}, check=[P[5], P[17], P["on"]])]   # seqQ 0 everywhere: every sumq ties at 0
    return B.finish("manytypes", runs=runs, keys=P)


def _zq(seed, unmapped):
    S = 3
    B = Builder(seed, S, 300 + 300 * 6)
    rng = B.rng
    for k in range(6):
        pos = 250 + 300 * k
        ty = (-2, 1, 3, -1, 2, -4)[k]
        B.site(pos, type=ty)
        for s in range(S):
            B.column(pos, s, int(rng.integers(10, 15)), [(ty, 3, None)])
    for rl in B.by:
        for j, r in enumerate(rl):
            if (j + int(rng.integers(0, 2))) % 2 == 0:
                continue                                        # r_has_zq mixed inside every column
            r.qual = rng.integers(0, 51, r.l_qseq).astype(np.int32)
            cat = rng.integers(0, 4, r.l_qseq)                  # qual + zq - 64 below 0, in 0..6, in 7..30, above 30
            tgt = rng.integers(np.array([-9, 0, 7, 31])[cat], np.array([-1, 6, 30, 80])[cat] + 1)
            r.zq = (tgt - r.qual + 64).astype(np.uint8)
    return B.finish("zq")


def _bigins(seed, unmapped):
    S = 4
    B = Builder(seed, S, 300 + 300 * 4)
    rng = B.rng
    for k, tys in enumerate(((65, 1, -1), (70, 2, -2), (100, 3, -3), (65, 70, 100))):
        pos = 250 + 300 * k
        B.site(pos, types=tys)
        ins = {t: B.rand(t) for t in tys if t > 0}
        for s in range(S):
            for j in range(int(rng.integers(11, 14))):
                t = tys[j % 3] if j < 4 else 0
                i = max(t, 0)
                off = int(rng.integers(10, 150 - i - 12))
                B.carrier(s, pos, 150, off, t, ins.get(t))
    return B.finish("bigins")


_SCEN = dict(cigars=_cigars, repeats=_repeats, refletters=_refletters, edges=_edges, mask=_mask, manytypes=_manytypes, zq=_zq, bigins=_bigins)


def scenario(name, seed, unmapped=True):
    """The batch of indeldrv (ref, reads, pos, smpl_off, p_read, p_qpos, p_indel, n_sites, n_smpl) plus: pool = (reads, r_mapq,
    r_smpl, None) for bcfgpu_pileup (the same reads), objs (the read objects in pool order), refseq (str), notes (per site),
    runs = [dict(kw = options of the stage, dead = sites designed to return -1, check = the sites to compare, None: all)],
    has_unmapped.  unmapped=False: the same reads with no flag 4 among them (bcfgpu_pileup takes filtered reads only)."""
    return _SCEN[name](int(seed), unmapped)
