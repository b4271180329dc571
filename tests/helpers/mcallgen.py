"""Caller inputs for tests/test_gpu_mcall_cohort.py and tests/test_oracle_mcall_cohort.py.

cohort_records(): stand-alone caller records (bcfgpu_call_in) at cohort scale, PLs from a per-read error model and
    not clipped, plus explicit entries at the edges of set_pdg's arithmetic (EDGE_PLS).
tie_records():    records symmetric under swapping two ALT alleles, so that subsets and genotypes tie exactly.
tie_tile():       a pileup tile whose cells hold equally many, attribute-for-attribute equal reads of two non-reference
                  bases (equal QS: the ALT order ties; symmetric PL planes: the caller ties).
"""
import numpy as np

from bcftools_amd import abi, host

MISSING, VEND = abi.INT32_MISSING, abi.INT32_VECTOR_END

# 255/256: the last table entry and the first pow(); 3077: 10^(-PL/10) is subnormal from here; 3237: it is 0 from here
EDGE_PLS = (255, 256, 257, 3076, 3077, 3236, 3237, 10000, 12345, 99999)
PL_SUBNORMAL, PL_ZERO = 3077, 3237


def gts_of(na):
    """(a, b) of every genotype in VCF order (b <= a)."""
    return [(a, b) for a in range(na) for b in range(a + 1)]


def diag(na):
    return [(a + 1) * (a + 2) // 2 - 1 for a in range(na)]


def _pls_from_reads(rng, n_smpl, na, depth, af, n_obs):
    """Per-read error model: a sample's genotype from `af` (HWE), Poisson(depth) reads each showing one of its two alleles,
    changed to another of the first `n_obs` alleles (no read shows an unseen <*>) with the read's error rate 10^(-Q/10),
    Q in {20, 30, 40}.  PL = -10 log10 L(G), minus the
    sample's minimum, rounded, unclipped.  Returns PL [n_gt][n_smpl] and allele counts [na][n_smpl]."""
    g = rng.choice(na, size=(n_smpl, 2), p=af)
    n = rng.poisson(depth, n_smpl)
    smp = np.repeat(np.arange(n_smpl), n)
    R = len(smp)
    true = g[smp, rng.integers(0, 2, R)]
    e = 10.0 ** (-rng.choice([20, 30, 40], size=R) / 10.0)
    obs = true.copy()
    if n_obs > 1:
        flip = rng.random(R) < e
        obs[flip] = (true[flip] + rng.integers(1, n_obs, int(flip.sum()))) % n_obs
    cnt = np.zeros((na, n_smpl), dtype=np.int64)
    np.add.at(cnt, (obs, smp), 1)
    L = np.zeros((na * (na + 1) // 2, n_smpl))
    for z, (a, b) in enumerate(gts_of(na)):
        pa = np.where(obs == a, 1 - e, e / 3)
        pb = np.where(obs == b, 1 - e, e / 3)
        L[z] = np.bincount(smp, weights=-10 * np.log10(0.5 * pa + 0.5 * pb), minlength=n_smpl)
    pl = np.round(L - L.min(axis=0)).astype(np.int64)
    return pl, cnt, n


def cohort_records(seed, n_sites, n_smpl, use_ploidy=False, n_grp=1, shuffled=False, use_prior=False, i16=True):
    """Stand-alone caller records at cohort scale.  Depth 8, 30 and 120 in turn; 1-5 alleles, the last one an unseen <*>
    (no read shows it) at about half the sites; PLs as a per-read error model gives them, thousands at depth 120, and at
    about one sample in eight one non-minimal entry replaced by one of EDGE_PLS (each sample keeps a 0).  Missing entries,
    all-missing samples, haploid / absent samples (ploidy 1 / 0), -G groups on FORMAT/AD (contiguous runs or shuffled),
    -F priors, INFO/I16 with counts in the thousands.

    Outside the contract, and so not generated: a sample with a missing entry and another entry >= 256 (set_pdg fills
    missing entries from the 256-entry pl2p table without a range check, mcall.c:522: undefined behaviour in the
    reference; the device's `& 255` is not a contract), a sample whose PLs are all >= 3237 (every likelihood is 0 and
    the reference divides by their sum), and a record whose called alleles include the unseen one (the reference writes
    GT/GP past nals_new): the unseen allele has no reads, so QS = 0, and its genotypes' PLs stay below 3077."""
    rng = np.random.default_rng(seed)
    nals = rng.integers(1, 6, n_sites).astype(np.int32)
    nals[:5] = [1, 2, 3, 4, 5][:n_sites]
    unseen = np.where(rng.random(n_sites) < 0.5, nals - 1, 0).astype(np.int32)
    unseen[nals <= 2] = 0
    ng = nals * (nals + 1) // 2
    n_gt_max = int(ng.max())                     # as bcfgpu_call.c sizes the PL planes: the batch's largest record
    ploidy = rng.choice([0, 1, 2, 2, 2, 2], size=n_smpl).astype(np.uint8) if use_ploidy else None
    pl = np.full((n_sites, n_gt_max, n_smpl), VEND, dtype=np.int32)
    qs = np.zeros((n_sites, 5), dtype=np.float32)
    ad = np.full((n_sites, 5, n_smpl), VEND, dtype=np.int32) if n_grp > 1 else None
    for k in range(n_sites):
        na, x = int(nals[k]), int(ng[k])
        depth = (8, 30, 120)[k % 3]
        af = rng.dirichlet(np.r_[4.0, np.full(na - 1, 1.0)]) if na > 1 else np.array([1.0])
        if unseen[k] > 0:
            af[unseen[k]] = 0.0
            af /= af.sum()
        # (with QS = 0 the unseen allele is never part of a candidate subset; if it were selected, the reference would index
        # GPs/gts past nals_new -- mcall.c:1571-1577 -- which is undefined behaviour, not something to test parity on)
        v, cnt, n = _pls_from_reads(rng, n_smpl, na, depth, af, na - 1 if unseen[k] > 0 else na)
        # explicit edge values: one non-minimal entry of about one sample in eight
        if x > 1:
            for s in np.nonzero(rng.random(n_smpl) < 0.125)[0]:
                cand = np.nonzero(v[:, s] > 0)[0]
                if len(cand) == 0:
                    cand = np.arange(1, x)
                v[rng.choice(cand), s] = rng.choice(EDGE_PLS)
        if unseen[k] > 0:
            # the single-allele row skips samples whose likelihood is 0 (mcall.c:600-611): with 0 for the unseen allele's
            # genotypes it could win, and then the reference indexes past nals_new (above).  Kept finite, it cannot.
            u = [z for z, (a, b) in enumerate(gts_of(na)) if unseen[k] in (a, b)]
            v[u] = np.minimum(v[u], PL_SUBNORMAL - 1)
        for s in range(n_smpl):
            pd = 2 if ploidy is None else int(ploidy[s])
            col = v[:, s].astype(np.int32)
            if n[s] == 0 and rng.random() < 0.5:
                col[:] = MISSING if rng.random() < 0.5 else 0
            elif pd == 2 and x > 1 and rng.random() < 0.05:
                col = np.minimum(col, 255)           # a missing entry: the sample's values stay in the table's range
                col[rng.integers(0, x)] = MISSING
            if pd == 1:
                col = np.r_[col[diag(na)], np.full(x - na, VEND, np.int32)] if x > na else col
            elif pd == 0:
                col = np.full(x, VEND, np.int32)
                col[0] = MISSING
            pl[k, :x, s] = col
        if ad is not None:
            ad[k, :na] = cnt
        q = (cnt * 30).sum(axis=1).astype(np.float64)
        if q.sum() > 0:
            qs[k, :na] = (q / q.sum()).astype(np.float32)
    grp = None
    if n_grp > 1:
        grp = (np.arange(n_smpl) * n_grp // n_smpl).astype(np.int32)
        if shuffled:
            rng.shuffle(grp)
    prior_an = prior_ac = None
    if use_prior:
        prior_an = np.full(n_sites, 2 * n_smpl, dtype=np.int32)
        prior_ac = np.full((n_sites, 4), VEND, dtype=np.int32)
        for k in range(n_sites):
            na = int(nals[k])
            if na > 1:
                prior_ac[k, :na - 1] = rng.multinomial(n_smpl // 2, np.full(na - 1, 1.0 / (na - 1)))
            if rng.random() < 0.2:
                prior_an[k] = MISSING
    i16a = None
    if i16:
        i16a = np.zeros((n_sites, 16), dtype=np.float32)
        for k in range(n_sites):
            cnt = rng.integers(0, 5000, 4) * (rng.random(4) < 0.85)
            i16a[k, :4] = cnt
            for t in range(3):
                for side, m in ((0, int(cnt[0] + cnt[1])), (1, int(cnt[2] + cnt[3]))):
                    w = rng.integers(0, 60, m)
                    i16a[k, 4 + 4 * t + 2 * side] = w.sum()
                    i16a[k, 5 + 4 * t + 2 * side] = (w * w).sum()
    return host.CallInput(n_smpl, nals, unseen, pl, qs, ad=ad, ploidy=ploidy, grp=grp, prior_an=prior_an,
                          prior_ac=prior_ac, i16=i16a)


# ---- exact ties ----
# Each kind: (nals, unseen, QS, tied ALT pair (lo, hi), sample types).  A sample type is (share, PL by genotype, AD): the PL
# vector of every type is symmetric under lo <-> hi, so is the AD, and lo and hi have equal QS.  A subset holding lo and
# its mirror holding hi then get bit-equal likelihoods in every sample, in the same sample order.
_H = 60                                           # a PL far from the best

def _pl(na, best, mid=(), midv=20):
    v = {gt: _H for gt in gts_of(na)}
    for gt in mid:
        v[gt] = midv
    for gt in best:
        v[gt] = 0
    return [v[gt] for gt in gts_of(na)]


TIE_KINDS = {
    # single {1} ties with {2}: every sample is 1/1 or 2/2 alike
    "single": (3, 0, [.1, .45, .45], (1, 2), [(1.0, _pl(3, [(1, 1), (2, 2)], [(1, 0), (2, 0)], 30), [1, 4, 4])]),
    # the same behind an allele of frequency 0
    "single_zf": (4, 0, [.1, 0, .45, .45], (2, 3), [(1.0, _pl(4, [(2, 2), (3, 3)], [(2, 0), (3, 0)], 30), [1, 0, 4, 4])]),
    # pair {0,1} ties with {0,2}: mostly 0/0, a fifth of the samples 0/1 and 0/2 alike
    "pair": (3, 0, [.8, .1, .1], (1, 2), [(0.8, _pl(3, [(0, 0)]), [8, 0, 0]), (0.2, _pl(3, [(1, 0), (2, 0)]), [4, 2, 2])]),
    "pair_zf": (4, 0, [.8, 0, .1, .1], (2, 3), [(0.8, _pl(4, [(0, 0)]), [8, 0, 0, 0]),
                                                 (0.2, _pl(4, [(2, 0), (3, 0)]), [4, 0, 2, 2])]),
    # with the unseen allele <*> last
    "pair_unseen": (4, 3, [.8, .1, .1, 0], (1, 2), [(0.8, _pl(4, [(0, 0)]), [8, 0, 0, 0]),
                                                     (0.2, _pl(4, [(1, 0), (2, 0)]), [4, 2, 2, 0])]),
    # triple {0,1,3} ties with {0,2,3}: 0/0, 0/3, and 0/1 = 0/2
    "triple": (4, 0, [.6, .1, .1, .2], (1, 2), [(0.5, _pl(4, [(0, 0)]), [8, 0, 0, 0]), (0.25, _pl(4, [(3, 0)]), [4, 0, 0, 4]),
                                                 (0.25, _pl(4, [(1, 0), (2, 0)]), [4, 2, 2, 0])]),
    # genotypes: {0,1,2} is called (0/1 and 0/2 samples in equal shares: the one sample type that is not symmetric by
    # itself, its AD is); samples with 0/1 = 0/2 or 1/1 = 2/2 tie
    "gt": (3, 0, [.5, .25, .25], (1, 2), [(0.3, _pl(3, [(1, 0)]), [4, 2, 2]), (0.3, _pl(3, [(2, 0)]), [4, 2, 2]),
                                           (0.2, _pl(3, [(1, 0), (2, 0)]), [4, 2, 2]),
                                           (0.2, _pl(3, [(1, 1), (2, 2)], [(1, 0), (2, 0)], 10), [0, 4, 4])]),
    # five alleles with a frequency each (the 25-subset instantiation): pair {0,2} ties with {0,3}
    "pair5": (5, 0, [.6, .1, .1, .1, .1], (2, 3), [(0.6, _pl(5, [(0, 0)]), [8, 0, 0, 0, 0]),
                                                    (0.2, _pl(5, [(2, 0), (3, 0)]), [4, 0, 2, 2, 0]),
                                                    (0.1, _pl(5, [(1, 0)], [], 40), [4, 2, 0, 0, 0]),
                                                    (0.1, _pl(5, [(4, 0)], [], 40), [4, 0, 0, 0, 2])]),
}


def _sample_types(n_smpl, types, rng):
    """Type of each sample: the shares rounded to counts, in a shuffled order."""
    cnt = [int(round(sh * n_smpl)) for sh, _, _ in types]
    cnt[0] += n_smpl - sum(cnt)
    t = np.repeat(np.arange(len(types)), cnt)
    rng.shuffle(t)
    return t


def mirror_gt(na, lo, hi):
    """Index of the genotype that swapping lo and hi makes of each genotype."""
    mirror = {a: a for a in range(na)}
    mirror[lo], mirror[hi] = hi, lo
    gts = gts_of(na)
    return [gts.index(tuple(sorted((mirror[a], mirror[b]), reverse=True))) for a, b in gts]


def symmetric_samples(cin, k, lo, hi):
    """Samples of record k whose PL vector is unchanged by swapping lo and hi (haploid and absent samples included)."""
    na = int(cin.nals[k])
    x = na * (na + 1) // 2
    v = cin.pl[k, :x]
    hap = (v[na:] == VEND).all(axis=0) if x > na else np.zeros(cin.n_smpl, bool)
    dip = (v == v[mirror_gt(na, lo, hi)]).all(axis=0)
    d = v[:na]
    hsym = d[lo] == d[hi]
    return np.where(hap, hsym, dip)


def later_without_earlier(gt, als_map, early, late):
    """Samples whose genotype (gt [2][n_smpl] of one record) holds the later allele of a tied pair but not the earlier one:
    where the two tie, the reference's strict `best_lk < lk` keeps the earlier genotype."""
    me, ml = int(als_map[early]), int(als_map[late])
    if ml < 0:
        return np.zeros(gt.shape[1], bool)
    return (gt == ml).any(axis=0) & ~(gt == me).any(axis=0)


def tie_records(seed, n_smpl, kinds=tuple(TIE_KINDS), reps=2, use_ploidy=False, n_grp=1, shuffled=False):
    """`reps` records of every kind in `kinds`, all at the largest nals among them (n_gt_max).  Per sample a symmetric
    amount (0-9) is added to the PLs of the genotypes holding neither tied allele and to those holding both, equal amounts
    to the mirrored ones: the samples differ, the symmetry stays.  Returns (CallInput, [kind of each record])."""
    rng = np.random.default_rng(seed)
    names = [k for k in kinds for _ in range(reps)]
    n_sites = len(names)
    n_gt_max = max(TIE_KINDS[k][0] * (TIE_KINDS[k][0] + 1) // 2 for k in kinds)
    ploidy = rng.choice([0, 1, 2, 2, 2], size=n_smpl).astype(np.uint8) if use_ploidy else None
    nals = np.zeros(n_sites, np.int32)
    unseen = np.zeros(n_sites, np.int32)
    qs = np.zeros((n_sites, 5), np.float32)
    pl = np.full((n_sites, n_gt_max, n_smpl), VEND, np.int32)
    ad = np.full((n_sites, 5, n_smpl), VEND, np.int32) if n_grp > 1 else None
    for k, name in enumerate(names):
        na, us, q, (lo, hi), types = TIE_KINDS[name]
        x = na * (na + 1) // 2
        nals[k], unseen[k] = na, us
        qs[k, :na] = np.asarray(q, np.float32)
        ty = _sample_types(n_smpl, types, rng)
        mgt = mirror_gt(na, lo, hi)
        for s in range(n_smpl):
            col = np.array(types[ty[s]][1], np.int64)
            add = rng.integers(0, 10, x)
            add = np.where(np.arange(x) < np.array(mgt), add[mgt], add)      # symmetric: the mirror gets the same amount
            col = col + np.where(col > 0, add, 0)
            pd = 2 if ploidy is None else int(ploidy[s])
            if pd == 1:
                col = np.r_[col[diag(na)], np.full(x - na, VEND)]
            elif pd == 0:
                col = np.r_[[MISSING], np.full(x - 1, VEND)]
            pl[k, :x, s] = col
            if ad is not None:
                ad[k, :na, s] = types[ty[s]][2]
    grp = None
    if n_grp > 1:
        grp = (np.arange(n_smpl) * n_grp // n_smpl).astype(np.int32)
        if shuffled:
            rng.shuffle(grp)
    return host.CallInput(n_smpl, nals, unseen, pl, qs, ad=ad, ploidy=ploidy, grp=grp), names


def tie_tile(seed, n_sites, n_smpl, ref_n=False, het=(0.04, 0.3)):
    """SNP tile in which every site has two tied non-reference bases lo < hi: a cell holds m reference reads and, in a
    share het[k % 2] of the cells (few: a pair of the tied base with the reference is called; more: the triple), k reads of lo and k of hi whose i-th reads have the same quality, mapQ, strand, tail, soft-clip
    flag and epos (k in 1..3, m = k + 2 .. k + 5, so that 0/lo = 0/hi beat lo/hi).  With `ref_n` the reference is N, the
    other two bases carry reads too (different counts, so only lo and hi tie) and the site has five alleles.
    Returns (HostTile, lo[n_sites], hi[n_sites]) in 0..3 base codes."""
    rng = np.random.default_rng(seed)
    S = n_smpl
    ref2 = rng.integers(0, 4, n_sites)
    lo = np.zeros(n_sites, np.int64)
    hi = np.zeros(n_sites, np.int64)
    rd, ep, nread = [], [], []

    def reads(base, bq, mq, strand, tail, sclip):
        return (bq | (mq << 8) | ((1 << base) << 16) | (strand << 20) | (sclip << 21) | (tail << 24)).astype(np.uint32)

    def attrs(n):
        bq = rng.choice([20, 25, 30, 37, 40], n)
        mq = rng.choice([20, 40, 60, 60], n)
        qpos = rng.integers(0, 150, n)
        return bq, mq, rng.integers(0, 2, n), np.minimum(qpos, 149 - qpos), (rng.random(n) < 0.05).astype(np.int64), \
            ((qpos + 1) / 151.0 * 100).astype(np.uint8)

    for k in range(n_sites):
        others = [b for b in range(4) if b != ref2[k]]
        pair = sorted(rng.choice(others, 2, replace=False))
        lo[k], hi[k] = pair
        rest = [b for b in range(4) if b not in pair]           # with ref_n: the two other bases, different counts
        for s in range(S):
            bq, mq, st, tl, sc, e = attrs(0)
            cell_rd, cell_ep = [], []
            if ref_n:
                for j, b in enumerate(rest):
                    n = int(rng.integers(0, 3)) + 3 * j      # never equal counts with the other one, nor both tied
                    a = attrs(n)
                    cell_rd.append(reads(b, *a[:5])); cell_ep.append(a[5])
            else:
                m = int(rng.integers(3, 9))
                a = attrs(m)
                cell_rd.append(reads(ref2[k], *a[:5])); cell_ep.append(a[5])
            if rng.random() < het[k % 2] or ref_n:
                kk = int(rng.integers(1, 4))
                a = attrs(kk)
                cell_rd.append(reads(lo[k], *a[:5])); cell_ep.append(a[5])
                cell_rd.append(reads(hi[k], *a[:5])); cell_ep.append(a[5])
            r = np.concatenate(cell_rd) if cell_rd else np.zeros(0, np.uint32)
            e = np.concatenate(cell_ep) if cell_ep else np.zeros(0, np.uint8)
            p = rng.permutation(len(r))
            rd.append(r[p]); ep.append(e[p]); nread.append(len(r))
    off = np.zeros(n_sites * S + 1, np.int64)
    np.cumsum(nread, out=off[1:])
    ref16 = np.where(ref_n, 15, 1 << ref2).astype(np.int8)
    return host.HostTile(S, ref16, off.astype(np.uint32), np.concatenate(rd), np.concatenate(ep)), lo, hi
