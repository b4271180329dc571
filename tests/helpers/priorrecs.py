"""Records for the tests of the caller's prior: the random records of tests/test_gpu_mcall_random.py with records among them
whose QUAL is the prior alone, the closed form of that QUAL, and a writer that turns such records into a VCF for bcfgpu_call.

A record that is called REF, with no ALT subset that any sample's likelihoods support, takes mcall.c:1641-1642:
QUAL = -4.343 * log(theta'), theta' = theta * (1 + sum_{i=2}^{n-1} 1/i) or 0.99 when that is >= 1, n = ploidy_max * samples
(mcall.c:396-416); QUAL = 0 without a prior.  No likelihood enters it.  Two shapes of record get there:
  nals == 1                    a PL above 0 (a sample whose PL sums to the number of genotypes counts as missing, mcall.c:531-536);
  nals == 2, ALT the unseen    QS of the ALT 0 (no two-allele subset is tried, mcall.c:622), and the ALT-homozygous PL so large
                               that 10^(-PL/10) is 0 in a double (past 3240; the single-allele loop of mcall.c:601-615 skips it).
"""
import math

import numpy as np

from bcftools_amd import abi, host

MISSING, VEND = abi.INT32_MISSING, abi.INT32_VECTOR_END
N_PRIOR_ONLY = 4


def prior_alleles(ploidy_max, n_smpl):
    return (ploidy_max if ploidy_max > 0 else 2) * n_smpl


def scaled_theta(theta, n):
    """theta' of mcall.c:396-416 before the logarithm, and whether the 0.99 cap took effect."""
    t = theta * (1.0 + sum(1.0 / i for i in range(2, n)))
    return (0.99, True) if t >= 1 else (t, False)


def prior_only_qual(theta, n):
    """QUAL of mcall.c:1642 as the float32 the record holds."""
    if not theta > 0:
        return np.float32(0)
    return np.float32(-4.343 * math.log(scaled_theta(theta, n)[0]))


def records(seed, n_random, n_smpl, use_ploidy):
    """(CallInput, indices of the prior-only records).  n_random random records of 1-5 alleles with N_PRIOR_ONLY prior-only
    records spread among them.  With a ploidy array the first sample that is not absent carries data at every prior-only record,
    so that AC[0] > 0 there; the seed moves on until the array has such a sample."""
    from tests.test_gpu_mcall_random import random_records
    n = n_random + N_PRIOR_ONLY
    while True:
        cin = random_records(seed, n, n_smpl, use_ploidy, 1, False)
        if cin.ploidy is None or cin.ploidy.any():
            break
        seed += 1000
    first = 0 if cin.ploidy is None else int(np.nonzero(cin.ploidy)[0][0])
    rng = np.random.default_rng(seed + 17)
    where = sorted({1 % n, n // 3, n // 2 + 1, n - 1})
    assert len(where) == N_PRIOR_ONLY
    for j, k in enumerate(where):
        cin.pl[k] = VEND
        cin.qs[k] = 0
        cin.qs[k, 0] = 1
        if j < 2:                                   # nals == 1: one PL a sample
            cin.nals[k], cin.unseen[k] = 1, 0
            v = rng.integers(1, 200, n_smpl)
            if j == 1:                              # some samples without data: PL 0 (sums to the genotype count) or missing
                v = np.where(rng.random(n_smpl) < 0.4, rng.choice([0, MISSING], n_smpl), v)
                v[first] = 37
            cin.pl[k, 0] = v
        else:                                       # REF and the unseen allele: 0 at genotype 0
            cin.nals[k], cin.unseen[k] = 2, 1
            cin.pl[k, 0] = 0
            cin.pl[k, 1] = rng.integers(3, 255, n_smpl) if j == 2 else rng.integers(3300, 5000, n_smpl)
            cin.pl[k, 2] = rng.integers(3300, 100000, n_smpl)
            if j == 3:                              # some samples wholly missing
                gone = rng.random(n_smpl) < 0.4
                gone[first] = False
                cin.pl[k, 0, gone] = MISSING
                cin.pl[k, 1:3, gone] = VEND
    return cin, np.array(where)


def select(cin, idx):
    """The records idx of a CallInput (one group, no -F prior)."""
    idx = np.asarray(idx)
    return host.CallInput(cin.n_smpl, cin.nals[idx], cin.unseen[idx], cin.pl[idx], cin.qs[idx], ploidy=cin.ploidy,
                          i16=None if cin.i16 is None else cin.i16[idx])


def assert_prior_only(res, where):
    """The records `where` of an oracle CallResult went the way the closed form describes: called, REF alone, a QUAL, REF alleles
    counted.  (That it was :1642 and not the likelihood ratio of :1640 is what the closed form itself then shows.)"""
    st = res.site[where]
    assert (st["ret"] > 0).all() and (st["als_new"] == 1).all() and (st["qual_missing"] == 0).all() and (st["ac"][:, 0] > 0).all(), st


VCF_HEADER = """##fileformat=VCFv4.2
##FILTER=<ID=PASS,Description="All filters passed">
##contig=<ID=17,length=100000>
##ALT=<ID=*,Description="Represents allele(s) other than observed.">
##INFO=<ID=I16,Number=16,Type=Float,Description="Auxiliary tag used for calling, see description of bcf_callret1_t in bam2bcf.h">
##INFO=<ID=QS,Number=R,Type=Float,Description="Auxiliary tag used for calling">
##FORMAT=<ID=PL,Number=G,Type=Integer,Description="List of Phred-scaled genotype likelihoods">
"""


def representable(cin):
    """The records write_vcf can spell: A and up to three other bases, besides <*>."""
    return np.nonzero(cin.nals - (cin.unseen > 0) <= 4)[0]


def write_vcf(cin, path, names, pos0=101):
    """The records of a CallInput as mpileup would have written them: REF A, the other alleles C, G, T in order with <*> at the
    unseen allele's index; INFO/QS, INFO/I16 where the input has it, FORMAT/PL.  Record k lies at 17:pos0 + k."""
    assert len(names) == cin.n_smpl
    with open(path, "w") as f:
        f.write(VCF_HEADER + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n")
        for k in range(cin.n_sites):
            na, un = int(cin.nals[k]), int(cin.unseen[k])
            bases = iter("CGT")
            alts = ["<*>" if un > 0 and i == un else next(bases) for i in range(1, na)]
            info = []
            if cin.i16 is not None:
                info.append("I16=" + ",".join("%d" % v for v in cin.i16[k]))
            info.append("QS=" + ",".join("%.9g" % v for v in cin.qs[k, :na]))
            cols = []
            for s in range(cin.n_smpl):
                v = []
                for x in cin.pl[k, :na * (na + 1) // 2, s]:
                    if x == VEND:
                        break
                    v.append("." if x == MISSING else str(int(x)))
                cols.append(",".join(v) if v else ".")
            f.write("17\t%d\t.\tA\t%s\t0\t.\t%s\tPL\t%s\n" % (pos0 + k, ",".join(alts) if alts else ".", ";".join(info), "\t".join(cols)))
