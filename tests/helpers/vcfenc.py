"""The sample columns of an mpileup record as VCF text, in Python, from the rules of the VCF specification (VCFv4.2, section
1.6.2 "Genotype fields"): per sample a tab, the FORMAT keys' values joined by ':', a key's values joined by ',', integers in
decimal.  Values here are non-negative and never missing (an mpileup record has no '.'), so a value's text is str(value).
Keys, widths and values come from tests/helpers/bcfenc.py (the same planes feed both encoders).  Test infrastructure: the
yardstick for bcfgpu_mplp_encode_vcf, itself pinned to the reference's goldens in tests/test_vcf_sample_text.py.
"""
import numpy as np

from tests.helpers.bcfenc import key_values, selected_keys

STAGE = 15 * 1024           # VCF_STAGE of vcfenc.hip: the bytes of text one round of the write kernel holds in LDS
SAMPLE_MAX = 293            # VCF_SAMPLE_MAX: eleven keys of five alleles with every plane at its largest value


def sample_text(fields, s):
    """fields: [vals [n_smpl][width]] in FORMAT order -> sample s's column, with the tab in front."""
    return b"\t" + b":".join(b",".join(b"%d" % v for v in f[s]) for f in fields)


def encode_site(fields):
    fields = [np.asarray(f, np.int64).tolist() for f in fields]
    return b"".join(sample_text(fields, s) for s in range(len(fields[0])))


def encode_planes(fmt_flag, n_alleles, pl, dp4, adf=None, adr=None, qs=None, scr=None, sp=None, emit=None):
    """What bcfgpu_mplp_encode_vcf is to produce from the planes of a tile ([site][plane][n_smpl], as bcfgpu_mplp_out):
    (bytes, offsets [n_sites + 1])."""
    n = len(n_alleles)
    keys = selected_keys(fmt_flag)
    out, off = [], np.zeros(n + 1, np.uint64)
    at = 0
    for k in range(n):
        if emit is None or emit[k]:
            g = lambda a: None if a is None else a[k]
            na = min(max(int(n_alleles[k]), 1), 5)
            b = encode_site([key_values(key, na, pl[k], dp4[k], g(adf), g(adr), g(qs), g(scr), g(sp)) for key in keys])
            out.append(b)
            at += len(b)
        off[k + 1] = at
    return np.frombuffer(b"".join(out), np.uint8), off
