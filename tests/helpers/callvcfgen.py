"""The generated inputs of tests/test_gpu_call_vcf_encode.py, numpy only so that tests/test_call_sample_text.py can check them
against the bound of include/bcfgpu.h without a device: 37 call records whose sample columns hold GT, an R key, PL (present or
dropped in turn), a one-value key, a third key that takes the paths of tests/test_gpu_call_key_encode.py in turn, and GQ; random
call planes with `missing`, early `end of vector` and haploid samples.  Test infrastructure."""
import numpy as np

from tests.helpers import callvcf
from tests.helpers.callenc import GT_MISSING, GT_VEND, MISSING, VEND
from tests.test_gpu_call_key_encode import N, key_values, narrow, sites

N_GT_MAX = 15


def call_planes(rng, site, S):
    """gt [n][2][S] int8, pl [n][15][S] int32, gq [n][S] int32: what bcfgpu_mcall could leave, and what it never does."""
    n = len(site)
    gt = np.zeros((n, 2, S), np.int8)
    pl = rng.integers(0, 256, (n, N_GT_MAX, S)).astype(np.int32)
    gq = rng.integers(0, 128, (n, S)).astype(np.int32)
    for r in range(n):
        nn = int(site["nals_new"][r])
        gt[r] = rng.integers(0, nn, (2, S))
        hap = rng.random(S) < (1.0 if r % 6 == 5 else 0.25 if r % 3 == 0 else 0.0)        # haploid samples: all, some, none
        gt[r, 1, hap] = GT_VEND
        gt[r, 0, rng.random(S) < 0.1] = GT_MISSING
        gt[r, 1, (rng.random(S) < 0.1) & ~hap] = GT_MISSING
        ngn = nn * (nn + 1) // 2
        for s in np.nonzero(hap)[0]:
            pl[r, nn:, s] = VEND                                    # a haploid sample's vector: one value per allele
        pl[r, ngn:, :] = VEND
        pl[r, rng.integers(0, ngn), rng.integers(0, S)] = MISSING
        pl[r, rng.integers(0, ngn), rng.integers(0, S)] = 70000 + r
        pl[r, rng.integers(0, ngn), rng.integers(0, S)] = -3 - r
        if r % 4 == 1:
            pl[r, 0, S // 2] = VEND                                 # ends at once: '.'
        if r % 4 == 2:
            pl[r, ngn - 1, 0] = VEND                                # one value short
        gq[r, rng.random(S) < 0.1] = MISSING
    return {"gt": gt, "pl": pl, "gq": gq}


def cases(S, seed=0, n=N):
    """(indiv bytes, fields of callvcf.FIELD_DTYPE, site records, planes, n_gt_max) for S input samples."""
    rng = np.random.default_rng(7000 * seed + S)
    site, nals = sites(n)
    site["pl_dropped"] = np.arange(n) % 2
    fields, buf = [], bytearray()
    n_key = [0]

    def plane(r, kind):
        fields.append((0, r, kind, 0, 0, 0, 0))

    def key(r, t, width, flags, vals):
        while len(buf) % 16 != n_key[0] % 16:
            buf.append(0xEE)
        n_key[0] += 1
        fields.append((len(buf), r, callvcf.KEY, t, width, int(nals[r]), flags))
        if t and width:
            buf.extend(narrow(vals, t))

    for r in range(n):
        a = int(nals[r])
        plane(r, callvcf.GT)
        t = 1 + r % 3
        key(r, t, a, 1, key_values(rng, S, a, t))
        if not site["pl_dropped"][r]:
            plane(r, callvcf.PL)
        t = 1 + (r + 1) % 3
        key(r, t if r % 6 else 0, 1 if r % 9 else 0, r % 2, key_values(rng, S, 1, t))
        kind = r % 7
        if kind == 0:                                               # an R key a value wider than the alleles: left alone
            key(r, 2, a + 1, 1, key_values(rng, S, a + 1, 2, sentinels=False))
        elif kind == 1:                                             # 130 values a sample, no R key
            key(r, 1, 130, 0, key_values(rng, S, 130, 1))
        elif kind == 2:                                             # int32 holding small values, padded with `end of vector`
            v = np.full((S, a + 2), VEND, np.int64)
            v[:, :a] = rng.integers(-100, 100, (S, a))
            key(r, 3, a + 2, 1, v)
        elif kind == 3:                                             # every sample missing
            v = np.full((S, a), VEND, np.int64)
            v[:, 0] = MISSING
            key(r, 2, a, 1, v)
        elif kind == 4:                                             # negative values
            v = key_values(rng, S, a, 3, sentinels=False)
            v[:] = np.minimum(v, 100)
            v[S // 2, a - 1] = (-120, -121, -32760, -2147483646)[(r // 7) % 4]
            key(r, 3, a, 1, v)
        elif kind == 5:                                             # 255 values of int32: the longest text a sample can have here
            key(r, 3, 255, 0, key_values(rng, S, 255, 3))
        else:
            key(r, 1, 15, 0, key_values(rng, S, 15, 1))
        if site["nals_new"][r] > 1 and site["ret"][r] > 0:
            plane(r, callvcf.GQ)
    buf.extend(b"\xEE" * 3)
    f = np.array(fields, dtype=callvcf.FIELD_DTYPE)
    return np.frombuffer(bytes(buf), np.uint8), f, site, call_planes(rng, site, S), N_GT_MAX
