"""The generated inputs of tests/test_gpu_call_vcf_rewrite.py, numpy only: call records of VCF text input whose sample columns hold
an R key, PL (first, in the middle, last or absent; listed or dropped in turn), a one-value Integer key, a Float key, a String key of
very unequal lengths and a second R key; columns that are '.' alone, have fewer or more tokens than the record has keys, empty
tokens, R tokens with one value more or fewer than the alleles or with empty values; any bytes between the records' runs, so that
the runs start at all 16 alignments.  The site records are those of tests/test_gpu_call_key_encode.py (nals cycling 1..5, alleles
dropped at the front, in the middle, at the end, all but the first, or not at all), the planes those of tests/helpers/callvcfgen.py.
Then the shapes that take the write kernel's other paths: a site past one round, columns and texts past a stage.  Test infrastructure."""
import numpy as np

from tests.helpers import callvcftext
from tests.helpers.callvcfgen import N_GT_MAX, call_planes
from tests.test_gpu_call_key_encode import sites

N = 40
STAGE = 15360                                                      # the LDS stages of the write kernel (BCFGPU_MAX_PL * 4 * 256)
_ALPHA = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789,;=|/._-+ ", np.uint8)


def string_token(rng, n):
    return _ALPHA[rng.integers(0, len(_ALPHA), n)].tobytes()


def r_token(rng, nals, how):
    """A Number=R token: one value an allele, or one of the forms that are left alone."""
    if how == 0:
        return b"."
    n = nals + (1 if how == 1 else -1 if how == 2 else 0)
    vals = [str(int(x)).encode() for x in rng.integers(-5, 3000, max(n, 0))]
    if how == 3 and vals:
        vals[int(rng.integers(0, len(vals)))] = b""               # an empty value keeps its place
    if how == 4 and vals:
        vals[int(rng.integers(0, len(vals)))] = b"."
    return b",".join(vals)


def pack(records):
    """records: dicts with cols (the input columns' bytes, without tabs), n_fmt, pl_idx, r_mask, nals, flags.  The text buffer with
    other bytes in front of every run, and the records of callvcftext.REC_DTYPE."""
    buf, rec = bytearray(), np.zeros(len(records), dtype=callvcftext.REC_DTYPE)
    for k, r in enumerate(records):
        buf += b"\n" * ((7 * k + 3 - len(buf)) % 16)               # run k starts at 7k + 3 mod 16: every alignment in 16 records
        run = b"".join(b"\t" + c for c in r["cols"])
        rec[k] = (len(buf), r["r_mask"], len(run), r["pl_idx"], r["n_fmt"], r["nals"], r["flags"])
        buf += run
    buf += b"\n\n\n"
    return np.frombuffer(bytes(buf), np.uint8), rec


def flags_of(site, r, pl_idx):
    called = site["nals_new"][r] > 1 and site["ret"][r] > 0
    return (callvcftext.FLAG_PL if pl_idx >= 0 and not site["pl_dropped"][r] else 0) | (callvcftext.FLAG_GQ if called else 0)


def cases(S, seed=0, n=N):
    """(text bytes, records of callvcftext.REC_DTYPE, site records, planes, n_gt_max) for S input samples."""
    rng = np.random.default_rng(9000 * seed + S)
    site, nals = sites(n)
    site["pl_dropped"] = (np.arange(n) // 2) % 2
    records = []
    for r in range(n):
        a = int(nals[r])
        keys = ["R", "I", "F", "S", "R"]                            # AD DP XF XS ADF
        place = r % 4                                               # PL first, in the middle, last, absent
        pl_idx = (0, 2, len(keys), -1)[place]
        if pl_idx >= 0:
            keys.insert(pl_idx, "PL")
        r_mask = sum(1 << i for i, k in enumerate(keys) if k == "R")
        lens = rng.integers(0, 40, S)
        lens[rng.random(S) < 0.15] = 0
        lens[rng.random(S) < 0.1] = int(rng.integers(200, 1500))
        if r % 8 == 5:
            lens += 250                                             # a record of long columns: past one round from 65 samples on
        cols = []
        for s in range(S):
            form = int(rng.integers(0, 12))
            if form == 0:
                cols.append(b".")                                   # the whole column '.'
                continue
            toks = []
            for k in keys:
                if k == "R":
                    toks.append(r_token(rng, a, int(rng.integers(0, 12)) if form != 1 else 5))
                elif k == "PL":
                    toks.append(b"0,1,2" if form % 2 else b".")   # (the input's PL is not what is written)
                elif k == "I":
                    toks.append(b"." if form == 2 else str(int(rng.integers(0, 100000))).encode())
                elif k == "F":
                    toks.append((b"0.125", b"-1.5e-07", b".", b"", b"3.40282e+38")[int(rng.integers(0, 5))])
                else:
                    toks.append(string_token(rng, int(lens[s])))
            if form == 3:
                toks = toks[:int(rng.integers(1, len(toks)))]       # fewer tokens than keys
            elif form == 4:
                toks += [b"more", string_token(rng, 9), b""]        # more tokens than keys
            elif form == 5:
                i = int(rng.integers(0, len(toks)))
                if keys[i] != "PL":                                 # (the input's PL stays something bcfgpu_call_decode_vcf reads)
                    toks[i] = b""                                   # an empty token
            cols.append(b":".join(toks))
        records.append(dict(cols=cols, n_fmt=len(keys), pl_idx=pl_idx, r_mask=r_mask, nals=a, flags=flags_of(site, r, pl_idx)))
    text, rec = pack(records)
    return text, rec, site, call_planes(rng, site, S), N_GT_MAX


def one_site(cols, seed=0, nals=3, keep=(0, 2)):
    """(text, rec, site, planes, n_gt_max) of one record with these input columns: keys R, PL, S; alleles 3 -> 2 (the middle one
    dropped), PL and GQ listed."""
    rng = np.random.default_rng(seed)
    site, _ = sites(1)
    m = [-1] * 5
    for new, old in enumerate(keep):
        m[old] = new
    site["nals_new"][0], site["als_map"][0], site["ret"][0], site["pl_dropped"][0] = len(keep), m, len(keep), 0
    text, rec = pack([dict(cols=cols, n_fmt=3, pl_idx=1, r_mask=1, nals=nals, flags=callvcftext.FLAG_PL | callvcftext.FLAG_GQ)])
    return text, rec, site, call_planes(rng, site, len(cols)), N_GT_MAX


def short_col(rng):
    return b"%d,%d,%d:.:%s" % (rng.integers(0, 99), rng.integers(0, 99), rng.integers(0, 99), string_token(rng, int(rng.integers(0, 30))))


def past_one_round(S=65):
    """One site whose input span and whose output each pass the stage at S samples: columns of about 300 bytes."""
    rng = np.random.default_rng(11)
    return one_site([b"1,2,3:0,0,0:" + string_token(rng, int(rng.integers(250, 350))) for _ in range(S)], seed=11)


def past_the_stage(which, S=1):
    """A column that takes the slow paths, alone (S == 1) or in the middle of short columns:
    "both"    a 20 000-byte String token: neither the column nor its text fits a stage
    "output"  a column of STAGE - 3 bytes (with its tab it fits the input stage) whose text, with GT, PL and GQ, does not
    "input"   20 000 bytes in tokens past the record's keys: they are dropped, the text is short"""
    rng = np.random.default_rng(13)
    if which == "both":
        long = b"7,8,9:.:" + string_token(rng, 20000)
    elif which == "output":
        long = b"7,8,9:.:" + string_token(rng, STAGE - 3 - 8)
        assert 1 + len(long) <= STAGE
    else:
        long = b"7,8,9:.:short:" + string_token(rng, 20000)
    cols = [short_col(rng) for _ in range(S)]
    cols[S // 2] = long
    return one_site(cols, seed=13)
