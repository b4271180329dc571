"""What bcfgpu_call_encode_bcf is to produce, in numpy / struct: FORMAT/GT, the trimmed FORMAT/PL and FORMAT/GQ of call records as
BCF2 key blocks, from the planes bcfgpu_mcall leaves and the site records.  The rules are those of the text route -- the VCF text
host/bcfgpu_call.c prints and host/vcfio.c encodes -- stated on the values:

    GT   per sample 1 or 2 allele indices; value (allele + 1) << 1, '.' -> 0; the record is as wide as its widest sample and a
         shorter sample ends with int8's `end of vector`; int8
    PL   a sample's vector is what is printed: its leading values up to the first `end of vector`, '.' when there is none; the
         record is as wide as its longest vector, shorter ones padded with `end of vector`; the smallest of int8 / int16 / int32
         that holds every value which is no sentinel (-120 .. 127, -32760 .. 32767)
    GQ   one value a sample, '.' = missing; typed as PL

A block is: the typed key id, the type / width descriptor, the values sample-major, little-endian.  Written from the BCF2
specification and the rules above, not from the kernel.  Test infrastructure: the yardstick for bcfgpu_call_encode_bcf (pinned
against the host writer in tests/test_call_indiv_encoder.py)."""
import struct

import numpy as np

MISSING, VEND = -2147483648, -2147483647
GT_MISSING, GT_VEND = -1, -2
KEYS = ("GT", "PL", "GQ")
_FMT = {1: "b", 2: "h", 3: "i"}
_SENT = {1: (-128, -127), 2: (-32768, -32767), 3: (MISSING, VEND)}


def typed_int(x):
    """A typed scalar that is no sentinel (a key id, a width)."""
    t = 1 if -120 <= x <= 127 else 2 if -32760 <= x <= 32767 else 3
    return bytes([0x10 | t]) + struct.pack("<" + _FMT[t], x)


def descriptor(width, t):
    return bytes([width << 4 | t]) if width < 15 else bytes([0xF0 | t]) + typed_int(width)


def int_type(values):
    """The BCF2 integer type (1, 2, 3) of a flat list of values; the sentinels do not decide it."""
    real = [v for v in values if v not in (MISSING, VEND)]
    if not real or (max(real) <= 127 and min(real) >= -120):
        return 1
    return 2 if max(real) <= 32767 and min(real) >= -32760 else 3


def encode_vectors(key_id, vecs, t=None):
    """vecs: per sample a list of values (MISSING / VEND allowed), of any lengths >= 1 -> the key's block."""
    width = max(len(v) for v in vecs)
    flat = [x for v in vecs for x in list(v) + [VEND] * (width - len(v))]
    if t is None:
        t = int_type(flat)
    miss, vend = _SENT[t]
    body = struct.pack("<%d%s" % (len(flat), _FMT[t]), *[miss if x == MISSING else vend if x == VEND else x for x in flat])
    return typed_int(key_id) + descriptor(width, t) + body


def gt_vectors(gt):
    """gt: [2][S] allele indices, GT_MISSING, GT_VEND -> per sample the BCF genotype values."""
    out = []
    for a, b in zip(*[[int(x) for x in row] for row in gt]):
        v = [0 if a in (GT_MISSING, GT_VEND) else (a + 1) << 1]
        if b != GT_VEND:
            v.append(0 if b == GT_MISSING else (b + 1) << 1)
        out.append(v)
    return out


def pl_vectors(pl, ngn):
    """pl: [>= ngn][S] -> per sample the printed vector: leading values up to the first VEND, [MISSING] when none."""
    out = []
    for s in range(pl.shape[1]):
        v = []
        for j in range(ngn):
            x = int(pl[j, s])
            if x == VEND:
                break
            v.append(x)
        out.append(v or [MISSING])
    return out


def encode_gt(key_id, gt):
    return encode_vectors(key_id, gt_vectors(gt), 1)


def encode_pl(key_id, pl, ngn):
    return encode_vectors(key_id, pl_vectors(np.asarray(pl), ngn))


def encode_gq(key_id, gq):
    return encode_vectors(key_id, [[int(x)] for x in gq])


def site_blocks(ids, nals_new, ret, pl_dropped, gt, pl, gq):
    """The three blocks (b"" = absent) of one site.  ids: {key: dictionary index}; pl / gq: planes or None."""
    nn = int(nals_new)
    ngn = nn * (nn + 1) // 2
    b_gt = encode_gt(ids["GT"], gt)
    b_pl = b"" if pl is None or pl_dropped else encode_pl(ids["PL"], pl, min(ngn, len(pl)))
    b_gq = encode_gq(ids["GQ"], gq) if gq is not None and nn > 1 and ret > 0 else b""
    return b_gt, b_pl, b_gq


def encode_planes(ids, site, gt, pl=None, gq=None, emit=None):
    """site: records with ret, nals_new, pl_dropped (a numpy record array or a list of dicts); gt [n][2][S], pl [n][n_gt_max][S],
    gq [n][S].  Returns (np.uint8 bytes, np.uint64 offsets [3 n + 1]): one offset per site and key, the last = the size."""
    if not isinstance(ids, dict):
        ids = dict(zip(KEYS, ids))
    data, off = bytearray(), [0]
    for k in range(len(site)):
        blocks = (b"", b"", b"")
        if emit is None or emit[k]:
            blocks = site_blocks(ids, site[k]["nals_new"], int(site[k]["ret"]), bool(site[k]["pl_dropped"]), gt[k],
                                 None if pl is None else pl[k], None if gq is None else gq[k])
        for b in blocks:
            data += b
            off.append(len(data))
    return np.frombuffer(bytes(data), np.uint8), np.array(off, np.uint64)


# ---- the values of a VCF text line, as the planes would hold them ----
def text_planes(fmt, samples):
    """fmt: the FORMAT column; samples: the sample columns.  Returns {key: plane} for the keys among GT, PL, GQ that the record has:
    GT [2][S] int8, PL [width][S] int32 padded with VEND, GQ [S] int32."""
    keys = fmt.split(":")
    cols = [s.split(":") for s in samples]
    S, out = len(cols), {}
    for i, key in enumerate(keys):
        vals = [c[i] if i < len(c) else "." for c in cols]
        if key == "GT":
            gt = np.full((2, S), GT_VEND, np.int8)
            for s, v in enumerate(vals):
                al = v.replace("|", "/").split("/")
                assert len(al) <= 2
                for j, a in enumerate(al):
                    gt[j, s] = GT_MISSING if a == "." else int(a)
            out[key] = gt
        elif key == "PL":
            vec = [[MISSING if x == "." else int(x) for x in v.split(",")] for v in vals]
            w = max(len(v) for v in vec)
            pl = np.full((w, S), VEND, np.int32)
            for s, v in enumerate(vec):
                pl[:len(v), s] = v
            out[key] = pl
        elif key == "GQ":
            out[key] = np.array([MISSING if v == "." else int(v) for v in vals], np.int32)
    return out
