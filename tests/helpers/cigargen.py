"""A second pileup reference and directed read pools for bcfgpu_pileup (test infrastructure).

tests/helpers/sam.walk answers "what is this read at this position" by walking the CIGAR from its start for every position --
the shape of the kernel's own walk.  expand_read goes over a CIGAR once, as htslib's stateful column iterator does, and emits
every reference position the read spans; what follows an aligned block comes from one backward pass over the operations.
expanded_pileup indexes positions once per read (not reads per position), which also makes it fast enough for 65 535-base
reads.  The rules are the published ones (htslib's resolve_cigar, as pileup.hip and sam.walk state them):
  M = X advance both coordinates; I S the query only; D N the reference only (is_del = 1, is_refskip = 1 for N, qpos = the next
  query base); H P nothing.  indel is non-zero only at the last base of an M = X block: pads after the block are skipped, a
  following I gives +len plus every further I reached through an unbroken run of I / P, a following D gives -len, an N gives 0.

MUTATIONS are single-rule changes of this reference, switched on by `mut`: tests/test_pileup_twins.py shows on the CPU that the
pools the GPU tests run on tell each of them from the rule.
"""
import functools
import re

import numpy as np

from bcftools_amd import abi, host
from . import sam
from .ovlfuzz import FuzzRead

MUTATIONS = ("pads_not_skipped", "ins_after_pad_dropped", "n_as_d", "indel_in_deletion", "tail_clamp_127", "iread_lt",
             "covers_end", "del_base_prev")

QUALS = np.array([2, 7, 11, 13, 20, 25, 30, 33, 37, 40, 41, 60], np.int32)       # at most 16 values: the packed forms' palette


# ---- the reference ---------------------------------------------------------------------------------------------------
def _after_block(cig, mut=None):
    """after[k] = the indel reported at the last base of an aligned block that ends just before operation k (one backward pass).
    run[k] = the I bases in the unbroken run of I / P that starts at k."""
    n = len(cig)
    after, run = [0] * (n + 1), [0] * (n + 1)
    for k in range(n - 1, -1, -1):
        l, op = cig[k]
        if op == "I":
            run[k] = l + run[k + 1]
            after[k] = run[k]
        elif op == "P":
            run[k] = 0 if mut == "ins_after_pad_dropped" else run[k + 1]
            after[k] = 0 if mut == "pads_not_skipped" else after[k + 1]
        elif op == "D" or (op == "N" and mut == "n_as_d"):
            after[k] = -l
    return after


def expand_read(read, lo=None, hi=None, mut=None):
    """(pos, qpos, is_del, is_refskip, indel) for every reference position the read spans, in one pass over its CIGAR;
    lo / hi: only the positions in [lo, hi)."""
    cig = read.cigar
    after = _after_block(cig, mut)
    x, y = read.pos, 0
    for k, (l, op) in enumerate(cig):
        if op in "M=X" or op in "DN":
            a, b, last = x, x + l, x + l - 1
            if lo is not None and lo > a:
                a = lo
            if hi is not None and hi < b:
                b = hi
            if op in "M=X":
                for p in range(a, b):
                    yield p, y + (p - x), 0, 0, after[k + 1] if p == last else 0
                y += l
            else:
                skip = 1 if op == "N" else 0
                for p in range(a, b):
                    yield p, y, 1, skip, after[k + 1] if (mut == "indel_in_deletion" and p == last) else 0
            x += l
        elif op in "IS":
            y += l
    if mut == "covers_end" and x > read.pos and (lo is None or lo <= x) and (hi is None or x < hi):
        yield x, y, 0, 0, 0


def aligned_position(read, qpos, mut=None):
    """bam2bcf.c:80-114 in closed form: (query offset + 1 less the soft clips that end at or before it, M = X I bases)."""
    y, edist, n_tot = 0, qpos + 1, 0
    for l, op in read.cigar:
        if op in "M=XI":
            n_tot += l
        if op in "M=XIS":
            y += l
        if op == "S" and (y < qpos if mut == "iread_lt" else y <= qpos):
            edist -= l
    return edist, n_tot


def expanded_pileup(reads_by_sample, refseq, beg, end, want_epos=True, mut=None):
    """The tile of [beg, end) -> (HostTile, col_n, col_indel, entries); entries[c] = [(read index in the pool, qpos, indel)] in
    (sample, read) order."""
    S, n_sites = len(reads_by_sample), end - beg
    cells = [[] for _ in range(n_sites * S)]
    ri = 0
    for si, rl in enumerate(reads_by_sample):
        for r in rl:
            rev, sclip = bool(r.flag & sam.BAM_FREVERSE), any(op == "S" for _, op in r.cigar)
            for pos, qpos, is_del, is_skip, indel in expand_read(r, beg, end, mut):
                qb = qpos - 1 if (mut == "del_base_prev" and is_del and qpos > 0) else qpos
                has = 0 <= qb < r.l_qseq
                w, e = sam.pack_read(sam.nt16(r.seq[qb]) if has else 15, int(r.qual[qb]) if has else 0, r.mapq, rev, sclip,
                                     is_del, is_skip, qpos, r.l_qseq, r.cigar, want_epos)
                if mut == "tail_clamp_127":
                    w = (w & 0x00ffffff) | min(w >> 24, 127) << 24
                if mut == "iread_lt" and want_epos:
                    ed, nt = aligned_position(r, qpos, mut)
                    e = min(max(int(float(ed) / (nt + 1) * 100), 0), 99)
                cells[(pos - beg) * S + si].append((w, e, ri, qpos, indel))
            ri += 1
    off = np.zeros(n_sites * S + 1, np.uint32)
    off[1:] = np.cumsum([len(c) for c in cells])
    flat = [t for c in cells for t in c]
    rd = np.array([t[0] for t in flat], np.uint32)
    ep = np.array([t[1] for t in flat], np.uint8)
    ref16 = np.array([sam.nt16(refseq[p]) if p < len(refseq) else 15 for p in range(beg, end)], np.int8)
    col_n = (off[S::S].astype(np.int64) - off[:-1:S]).astype(np.int32)
    entries = [[t[2:] for s in range(S) for t in cells[c * S + s]] for c in range(n_sites)]
    col_indel = np.array([int(any(t[2] != 0 for t in col)) for col in entries], np.uint8)
    return host.HostTile(S, ref16, off, rd, ep), col_n, col_indel, entries


# ---- directed reads --------------------------------------------------------------------------------------------------
def parse_cigar(s):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", s)]


def make_read(rng, pos, cigar, name=""):
    """A read with the fields of ovlfuzz.FuzzRead (pos, cigar, bamcigar, seq, qual, mapq, flag, l_qseq, end); cigar: text or list."""
    r = FuzzRead()
    r.cigar = parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
    r.pos, r.name, r.qname = int(pos), name, name
    r.l_qseq = sum(n for n, op in r.cigar if op in "M=XIS")
    r.end = r.pos + sum(n for n, op in r.cigar if op in "M=XDN")
    r.bamcigar = np.array([n << 4 | sam.CIG_OPS.index(op) for n, op in r.cigar], dtype=np.uint32)
    r.seq = "".join(np.array(list("ACGTN"))[rng.choice(5, r.l_qseq, p=[0.26, 0.26, 0.23, 0.23, 0.02])])
    r.qual = QUALS[rng.integers(0, len(QUALS), r.l_qseq)]
    r.mapq = int(rng.integers(0, 61))
    r.flag = int(rng.choice([0, 16]))
    return r


CLASSES = (
    # plain and flanks
    ("M", "12M"), ("EQ", "9="), ("X", "7X"), ("EQ_X_blocks", "4=2X5="),
    ("S_M", "3S9M"), ("M_S", "9M3S"), ("S_M_S", "2S8M3S"), ("H_M", "2H9M"), ("M_H", "9M2H"), ("H_S_M_S_H", "2H2S8M3S1H"),
    # leading and trailing I / D / N
    ("I_M", "2I8M"), ("S_I_M", "2S2I8M"), ("M_I", "8M2I"), ("M_I_S", "8M2I3S"), ("D_M", "2D8M"), ("M_D", "8M2D"), ("M_N", "8M3N"),
    # adjacent and padded operations
    ("M_I_M", "5M2I5M"), ("M_D_M", "5M2D5M"), ("M_N_M", "5M6N5M"),
    ("M_P_I_P_I_M", "4M1P2I1P1I4M"), ("M_I_I_M", "4M2I2I4M"), ("M_P_D_M", "4M1P2D4M"), ("M_I_D_M", "4M2I2D4M"), ("M_D_I_M", "4M2D2I4M"),
    # runs and the soft-clip rule
    ("M1I1_255ops", "1M1I" * 127 + "1M"),
    ("M_blocks_of_1", "1M1I1M1D1M1I1I1M2N1M1P1I1M1P1D1M1D1I1M1=1X1M"),
    ("S_I_M_D_M_S", "2S2I3M1D2M3S"), ("S_M_I_M_S", "3S4M2I4M2S"),
    # no reference span at all: in the candidate window of every later column, in no column
    ("S_only", "4S"), ("I_only", "3I"),
)
SHORT_SHAPES = tuple(c for n, c in CLASSES if n not in ("M1I1_255ops", "S_only", "I_only"))


def cigar_classes(pos0=20, step=3, seed=101):
    """One read per class of CLASSES (r.name), at ascending positions pos0, pos0 + step, ..."""
    rng = np.random.default_rng(seed)
    return [make_read(rng, pos0 + i * step, c, n) for i, (n, c) in enumerate(CLASSES)]


def _many_ops_cigar(l_qseq, n_blocks):
    """~2 * n_blocks operations: blocks of M / = / X with I, D, N, P I and I D between them, l_qseq query bases in all."""
    gaps = ([(3, "I")], [(2, "D")], [(7, "N")], [(1, "P"), (2, "I")], [(1, "I"), (4, "D")], [(1, "D")])
    ops, left = [(5, "S")], l_qseq - 5 - 4
    m = left // n_blocks - 2
    for i in range(n_blocks - 1):
        ops.append((m + i % 3, "M=X"[i % 7 % 3] if i % 7 < 3 else "M"))
        left -= m + i % 3
        for l, op in gaps[i % len(gaps)]:
            ops.append((l, op))
            if op == "I":
                left -= l
    return ops + [(left, "M"), (4, "S")]


def long_reads(pos0=100, seed=102):
    """Single-M reads of 255 ... 65 535 bases (the tail clamp at 255, the 16-bit lq / ntot fields at their last value), a
    5 000-base read with about 200 operations, and 30M20000N30M; at ascending positions from pos0."""
    rng = np.random.default_rng(seed)
    out = [make_read(rng, pos0 + i, "%dM" % n, "M%d" % n) for i, n in enumerate((255, 256, 257, 511, 512, 513, 5000, 65535))]
    out.append(make_read(rng, pos0 + 8, _many_ops_cigar(5000, 86), "ops200"))
    out.append(make_read(rng, pos0 + 9, "30M20000N30M", "skip20000"))
    return out


def too_long_read(pos=30, seed=103):
    return make_read(np.random.default_rng(seed), pos, "65536M", "M65536")


def too_many_ops_read(pos=30, seed=104):
    return make_read(np.random.default_rng(seed), pos, "1M1I" * 128, "M1I1_256ops")


def tie_reads(pos=60, seed=105):
    """dict(same_pos = 40 reads of one sample at one position with different lengths, pools = {n: a pool of exactly n reads})."""
    rng = np.random.default_rng(seed)
    same = [make_read(rng, pos, "%dM1D%dM" % (2 + i // 2, 1 + i - i // 2) if i % 4 == 3 else "%dM" % (3 + i), "tie%d" % i) for i in range(40)]
    four = [make_read(rng, pos, "7M", "p0"), make_read(rng, pos, "3M1I4M", "p1"), make_read(rng, pos + 2, "9M", "p2"),
            make_read(rng, pos + 3, "2S6M", "p3")]
    return dict(same_pos=same, pools={n: four[:n] for n in (1, 2, 3, 4)})


def random_ref(rng, n):
    return "".join(np.array(list("ACGTNRacgt"))[rng.choice(10, n, p=[0.2, 0.2, 0.2, 0.2, 0.02, 0.02, 0.04, 0.04, 0.04, 0.04])])


# ---- the pools of the GPU cases (tests/test_gpu_pileup_shapes.py; their coverage is asserted in tests/test_pileup_twins.py) ----
class Case:
    def __init__(self, name, by_sample, refseq, regions):
        self.name, self.by_sample, self.refseq, self.regions = name, by_sample, refseq, regions
        for rl in by_sample:
            assert all(a.pos <= b.pos for a, b in zip(rl, rl[1:])), "a sample's reads are in position order"

    @property
    def pool(self):
        return [r for rl in self.by_sample for r in rl]


def case_classes():
    """Case 1: the classes over 3 samples, the second holding one read and nothing else; from before the first read to past the last."""
    reads = cigar_classes()
    by_sample = [[r for i, r in enumerate(reads) if i != 4 and i % 2 == 0], [reads[4]], [r for i, r in enumerate(reads) if i % 2 == 1]]
    end = max(r.end for r in reads)
    return Case("classes", by_sample, random_ref(np.random.default_rng(1), end - 3), [(reads[0].pos - 6, end + 5)])


def case_window():
    """Case 3: one read with a 20 000-base skip first in its sample (max_span far above every other read's length), short reads
    starting inside the skip, a sample of short reads only and one of 40 reads at one position."""
    rng = np.random.default_rng(3)
    long_ = make_read(rng, 50, "30M20000N30M", "skip20000")
    far = ("1M1I" * 127 + "1M", "60M5D40M", "3S80M2I30M", "50M30N40M")
    s0 = [long_]
    for g, (a, b) in enumerate(((80, 120), (10030, 10110), (20000, 20060), (20061, 20079))):
        pos = np.sort(rng.integers(a, b + 1, 75))
        s0 += [make_read(rng, p, (far if g == 3 else SHORT_SHAPES)[i % (4 if g == 3 else len(SHORT_SHAPES))], "w%d_%d" % (g, i))
               for i, p in enumerate(pos)]
    regions = [(60, 124), (10050, 10114), (20050, 20114), (20112, 20176)]
    s1 = []
    for a, b in regions:
        pos = np.sort(rng.integers(a - 8, b, 20))
        s1 += [make_read(rng, p, SHORT_SHAPES[int(rng.integers(0, len(SHORT_SHAPES)))], "s1") for p in pos]
    s1.sort(key=lambda r: r.pos)
    s2 = tie_reads(pos=10070)["same_pos"]
    return Case("window", [s0, s1, s2], random_ref(rng, 400), regions)


def case_long():
    """Case 4: long_reads() in 2 samples; windows at the start, around qpos 254-257, at the middle and the last base of the
    65 535-base read, and across the ends and operations of the others."""
    reads = long_reads()
    by_sample = [reads[0::2], reads[1::2]]
    r64k = next(r for r in reads if r.name == "M65535")
    p0 = reads[0].pos
    regions = [(p0 - 8, p0 + 40), (p0 + 240, p0 + 288), (p0 + 490, p0 + 538), (p0 + 2480, p0 + 2528), (p0 + 4990, p0 + 5038),
               (r64k.pos + 32760, r64k.pos + 32808), (r64k.end - 40, r64k.end + 8), (p0 + 20050, p0 + 20098)]
    return Case("long", by_sample, random_ref(np.random.default_rng(4), 700), regions)


SHAPES = ((1, 1), (15, 15), (16, 16), (17, 17), (16, 33), (33, 16), (112, 5), (128, 5), (129, 5), (130, 129))


def case_shape(n_sites, S, beg=41):
    """Case 5: short reads of the classes' shapes; beg > 0, reads that start before beg and run past end, every fifth sample empty,
    a sample with no read at the first and the last column."""
    rng = np.random.default_rng(1000 * n_sites + S)
    end = beg + n_sites
    by_sample = []
    for s in range(S):
        if s % 5 == 2:
            by_sample.append([])
        elif s == 1:
            by_sample.append([make_read(rng, p, "%dM" % max(1, min(4, end - 1 - p)), "inner") for p in range(beg + 1, end - 1, 5)])
        else:
            pos = [beg - 4] * (s % 2 == 0) + sorted(int(p) for p in rng.integers(beg - 9, end + 1, 2 + s % 3)) + [end - 3] * (s % 3 == 0)
            by_sample.append([make_read(rng, p, SHORT_SHAPES[int(rng.integers(0, len(SHORT_SHAPES)))], "s%d" % s) for p in sorted(pos)])
    return Case("shape_%dx%d" % (n_sites, S), by_sample, random_ref(rng, end - 2), [(beg, end)])


def case_tie_pools():
    """Case 5: pools of exactly 1, 2, 3 and 4 reads in one sample (odd and even candidate counts; the pool's last read a candidate)."""
    t = tie_reads()
    ref = random_ref(np.random.default_rng(5), 90)
    return [Case("pool_of_%d" % n, [t["pools"][n]], ref, [(58, 74)]) for n in (1, 2, 3, 4)]


def case_three_in_order(x=18):
    """Case 5: position x under three reads in order -- one that ends before x, one that covers x through a D, one that covers it plainly."""
    rng = np.random.default_rng(6)
    rl = [make_read(rng, 10, "5M", "ends_before"), make_read(rng, 12, "4M6D4M", "through_D"), make_read(rng, 16, "8M", "plain")]
    return Case("three_in_order", [rl], random_ref(rng, 40), [(8, 30)])


def case_staging(extra):
    """Case 6: 16 samples x 36 single-M reads over exactly columns 0-15 = 9216 entries in the first workgroup (its LDS staging's
    capacity); extra = 1: one more 1-base read in one sample, 9217 (the lanes store straight to the tile).  Columns 16-31 are shallow."""
    rng = np.random.default_rng(7)
    by_sample = []
    for s in range(16):
        rl = [make_read(rng, 0, "16M", "deep") for _ in range(36)]
        if extra and s == 9:
            rl.append(make_read(rng, 5, "1M", "one_more"))
        rl += [make_read(rng, p, SHORT_SHAPES[(s + p) % len(SHORT_SHAPES)], "shallow") for p in range(16 + s % 3, 30, 4)]
        by_sample.append(rl)
    return Case("staging_%d" % (9216 + extra), by_sample, random_ref(rng, 32), [(0, 32)])


# an Euler circuit over (chunk start mod 4) x (chunk length mod 4): every pair once in 16 columns, back at the start after them
ALIGN_CIRCUIT = (3, 3, 3, 3, 2, 2, 1, 2, 2, 0, 1, 0, 1, 0, 1, 0)


def case_alignment():
    """Case 6: S = 2, the depth of column c chosen so that the columns' chunks of the epos bytes meet every (start mod 4, length
    mod 4); lengths 1, 2, 3 and 4 in columns 0-15, 5-8 in columns 16-31.  Every read covers one column (aI 1M bI: the epos byte
    depends on a and b)."""
    rng = np.random.default_rng(8)
    by_sample = [[], []]
    for c in range(32):
        d = (ALIGN_CIRCUIT[c % 16] or 4) + (4 if c >= 16 else 0)
        for j in range(d):
            a, b = int(rng.integers(0, 7)), int(rng.integers(0, 7))
            by_sample[(c + j) % 2 if d > 1 else c % 2].append(make_read(rng, c, "%dI" % a * (a > 0) + "1M" + "%dI" % b * (b > 0), "col%d" % c))
    return Case("alignment", by_sample, random_ref(rng, 32), [(0, 32)])


@functools.lru_cache(maxsize=None)
def cases():
    """Every pool the GPU tests run, by name; built once."""
    cs = ([case_classes(), case_window(), case_long()] + [case_shape(n, S) for n, S in SHAPES] + case_tie_pools() +
          [case_three_in_order(), case_staging(0), case_staging(1), case_alignment()])
    return {c.name: c for c in cs}


@functools.lru_cache(maxsize=None)
def reference(name, region=0, want_epos=True, mut=None):
    """expanded_pileup of a case's region, computed once and shared (nobody writes to it)."""
    c = cases()[name]
    beg, end = c.regions[region]
    return expanded_pileup(c.by_sample, c.refseq, beg, end, want_epos, mut)
