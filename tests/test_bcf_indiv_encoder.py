"""tests/helpers/bcfenc.py -- the numpy encoder of a record's per-sample part that the device encoder
(bcfgpu_mplp_encode_bcf) is compared with -- pinned against the host writer (host/vcfio.c encode_record) on the reference's
mpileup goldens: every record's FORMAT values, parsed from the VCF text and encoded here, must be the l_indiv bytes the
writer puts into the BCF form of the same file.  Then known answers at the places where the layout changes: the 15-wide
descriptor, the type boundaries, the three sizes of a key id.  CPU only."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests.helpers import bcfenc, vcf
from tests.test_c_host import VIEW_EXE, build_host

GOLDENS = ["mpileup.2.out", "mpileup.4.out", "mpileup.5.out", "mpileup.11.out", "indel-AD.1.out"]


def bcf_records(bcf):
    """(header text, [(shared bytes, indiv bytes)]) of an uncompressed BCF2 stream."""
    assert bcf[:5] == b"BCF\x02\x02"
    l_text, = struct.unpack_from("<I", bcf, 5)
    text = bcf[9:9 + l_text].split(b"\0")[0].decode()
    at, recs = 9 + l_text, []
    while at < len(bcf):
        l_shared, l_indiv = struct.unpack_from("<II", bcf, at)
        recs.append((bcf[at + 8:at + 8 + l_shared], bcf[at + 8 + l_shared:at + 8 + l_shared + l_indiv]))
        at += 8 + l_shared + l_indiv
    assert at == len(bcf)
    return text, recs


def format_ids(text):
    """{FORMAT key: dictionary index} from the IDX attributes of a BCF header."""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^##FORMAT=<ID=([^,]+),.*?IDX=(\d+)>$", text, flags=re.M)}


@pytest.mark.parametrize("goldf", GOLDENS)
def test_numpy_encoder_gives_the_writers_bytes_on_the_goldens(golden_dir, goldf):
    build_host()
    path = os.path.join(golden_dir, "mpileup", goldf)
    bcf = subprocess.run([VIEW_EXE, "-O", "u", path], check=True, stdout=subprocess.PIPE).stdout
    text, recs = bcf_records(bcf)
    ids = format_ids(text)
    gold = vcf.Vcf(path).recs
    assert len(gold) == len(recs) > 0
    widths = set()
    for r, (_, indiv) in zip(gold, recs):
        fields = []
        for k, key in enumerate(r.fmt_keys):
            vals = [[int(x) for x in s[k].split(",")] for s in r.smpl]
            fields.append((ids[key], vals))
            widths.add(len(vals[0]))
        assert bcfenc.encode_fields(fields) == indiv, r.line
    assert 3 in widths                       # (PL of REF and <*>)


def test_known_answers_at_the_layouts_seams():
    e = bcfenc
    # a key id of 127, 128 and 300: int8, int16, int16
    assert e.typed_int(5) == b"\x11\x05" and e.typed_int(127) == b"\x11\x7f"
    assert e.typed_int(128) == b"\x12\x80\x00" and e.typed_int(300) == b"\x12\x2c\x01"
    assert e.typed_int(32768) == b"\x13\x00\x80\x00\x00"
    # the descriptor: 14 values fit the high four bits, 15 do not (PL of five alleles)
    assert e.descriptor(14, 1) == b"\xe1" and e.descriptor(15, 1) == b"\xf1\x11\x0f" and e.descriptor(15, 2) == b"\xf2\x11\x0f"
    assert e.descriptor(1, 3) == b"\x13"
    # the type of a field is that of its largest value, whichever sample holds it
    assert e.encode_key(5, [[0, 127], [1, 2]]) == b"\x11\x05\x21" + bytes([0, 127, 1, 2])
    assert e.encode_key(5, [[0, 1], [128, 2]]) == b"\x11\x05\x22" + struct.pack("<4h", 0, 1, 128, 2)
    assert e.encode_key(5, [[32767], [0]]) == b"\x11\x05\x12" + struct.pack("<2h", 32767, 0)
    assert e.encode_key(5, [[0], [32768]]) == b"\x11\x05\x13" + struct.pack("<2i", 0, 32768)
    assert e.encode_key(300, [[255]]) == b"\x12\x2c\x01\x12\xff\x00"
    pl15 = np.arange(30).reshape(2, 15)
    assert e.encode_key(128, pl15) == b"\x12\x80\x00\xf1\x11\x0f" + bytes(range(30))


def test_planes_to_blocks():
    """encode_planes: key order and widths by allele count, AD = ADF + ADR, DP = the sum of DP4, the emit mask and offsets."""
    from bcftools_amd import abi
    S, n = 2, 3
    pl = np.zeros((n, 15, S), np.uint8); pl[:, 0] = (7, 9)
    dp4 = np.ones((n, 4, S), np.uint16); dp4[1, 3, 1] = 200
    adf = np.full((n, 5, S), 3, np.uint16); adr = np.full((n, 5, S), 4, np.uint16)
    ids = {k: 10 + i for i, k in enumerate(bcfenc.KEYS)}
    data, off = bcfenc.encode_planes(abi.FMT_DP | abi.FMT_AD, ids, [1, 2, 2], pl, dp4, adf=adf, adr=adr, emit=[1, 1, 0])
    b0 = b"\x11\x0a\x11\x07\x09" + b"\x11\x0b\x11\x04\x04" + b"\x11\x11\x11\x07\x07"
    b1 = b"\x11\x0a\x31\x07\x00\x00\x09\x00\x00" + b"\x11\x0b\x12" + struct.pack("<2h", 4, 203) + b"\x11\x11\x21" + bytes([7] * 4)
    assert bytes(data) == b0 + b1
    assert off.tolist() == [0, len(b0), len(b0) + len(b1), len(b0) + len(b1)]
