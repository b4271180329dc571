"""What bcfgpu_call_remap_bcf is to produce, in numpy / struct: the integer pass-through FORMAT keys of a call record (AD, ADF, ADR,
DP, SP, ...) as BCF2 key blocks, from the input record's bytes, the sample map and the site record's als_map.  The rule is the text
route's -- host/vcfio.c vio_indiv_text, the record loop of host/bcfgpu_call.c with print_numberR, host/vcfio.c encode_fmt_key /
enc_vint -- stated on the values:

    vector   a sample's `width` values widened (int8 / int16 `missing` and `end of vector` become the int32 sentinels), cut at the
             first `end of vector`; an empty one is the one value `missing`, the '.' of the text
    remap    Number=R, alleles dropped (nals_new != nals) and one value per allele: [v[0]] when one allele is left, else nals_new
             values `missing` with out[als_map[i]] = v[i] for the kept alleles; every other vector stays as it is
    block    the record is as wide as its longest vector, shorter ones padded with `end of vector`; the smallest of int8 / int16 /
             int32 that holds every value which is no sentinel (-120 .. 127, -32760 .. 32767); typed key id, descriptor, values

Written from the rule and the BCF2 specification, not from the kernel; the block layout is tests/helpers/callenc.py's.  Test
infrastructure: the yardstick for bcfgpu_call_remap_bcf (pinned against the host writer and the reference's goldens in
tests/test_call_key_encoder.py)."""
import numpy as np

from tests.helpers.callenc import MISSING, VEND, encode_vectors

SIZE = {0: 0, 1: 1, 2: 2, 3: 4}
_DT = {1: "<i1", 2: "<i2", 3: "<i4"}
_SENT = {1: (-128, -127), 2: (-32768, -32767), 3: (MISSING, VEND)}
# bcfgpu_bcf_key as a numpy record (bcftools_amd.abi.BCF_KEY, restated: the twin stands alone)
KEY_DTYPE = [("off", "<u8"), ("site", "<i4"), ("key_id", "<i4"), ("type", "<i4"), ("width", "<i4"), ("nals", "<i4"), ("flags", "<i4")]


def widen(raw, t, width, n_smpl_in):
    """The n_smpl_in x width values of a run of bytes as Python ints, the narrow types' sentinels widened."""
    if t == 0 or width == 0:
        return [[] for _ in range(n_smpl_in)]
    a = np.frombuffer(bytes(raw[:n_smpl_in * width * SIZE[t]]), _DT[t]).astype(np.int64).reshape(n_smpl_in, width)
    miss, vend = _SENT[t]
    return [[MISSING if x == miss else VEND if x == vend else int(x) for x in row] for row in a]


def sample_vector(vals):
    """Cut at the first `end of vector`; nothing left: one `missing`."""
    v = []
    for x in vals:
        if x == VEND:
            break
        v.append(x)
    return v or [MISSING]


def remap(v, is_r, nals, nn, als_map):
    """A Number=R vector with one value per allele follows the alleles; anything else stays."""
    if not (is_r and nn != nals and len(v) == nals):
        return list(v)
    if nn == 1:
        return [v[0]]
    out = [MISSING] * nn
    for i in range(nals):
        if als_map[i] >= 0:
            out[als_map[i]] = v[i]
    return out


def output_vectors(raw, t, width, n_smpl_in, nals, flags, nn, als_map, col=None, n_smpl=None):
    """Per called sample the vector the written record holds."""
    rows = widen(raw, t, width, n_smpl_in)
    cols = list(col) if col is not None else list(range(n_smpl_in if n_smpl is None else n_smpl))
    return [remap(sample_vector(rows[c]), flags & 1, nals, nn, als_map) for c in cols]


def encode_key(key_id, raw, t, width, n_smpl_in, nals=1, flags=0, nn=None, als_map=None, col=None, n_smpl=None):
    """One key's block.  nn / als_map default to "no allele dropped"."""
    if nn is None:
        nn, als_map = nals, list(range(nals))
    return encode_vectors(key_id, output_vectors(raw, t, width, n_smpl_in, nals, flags, nn, als_map, col, n_smpl))


def encode_jobs(indiv, keys, n_smpl_in, site, n_smpl, col=None, emit=None):
    """indiv: the byte buffer; keys: records of KEY_DTYPE; site: records with nals_new and als_map.  Returns (np.uint8 bytes,
    np.uint64 offsets [n_keys + 1])."""
    indiv = bytes(indiv)
    data, off = bytearray(), [0]
    for k in keys:
        s = int(k["site"])
        if emit is None or emit[s]:
            nn = min(max(int(site[s]["nals_new"]), 1), 5)
            data += encode_key(int(k["key_id"]), indiv[int(k["off"]):], int(k["type"]), int(k["width"]), n_smpl_in, int(k["nals"]), int(k["flags"]),
                               nn, [int(x) for x in site[s]["als_map"]], col, n_smpl)
        off.append(len(data))
    return np.frombuffer(bytes(data), np.uint8), np.array(off, np.uint64)
