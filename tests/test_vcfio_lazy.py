"""host/vcfio.c's record reading in two halves -- vio_read_record (the first nine columns and the raw per-sample block) and
vio_indiv_text (the block's sample columns as text) -- through `bcfgpu_view --lazy`: the head plus the text is the line
vio_read_line gives, on every golden turned into BCF; text input is refused.  CPU only."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW = os.path.join(ROOT, "host", "bcfgpu_view")


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "bcfgpu_view"])


def goldens(golden_dir):
    fs = sorted(glob.glob(os.path.join(golden_dir, "mpileup", "*.out")) + glob.glob(os.path.join(golden_dir, "call", "*.out")) +
                glob.glob(os.path.join(golden_dir, "call", "*.vcf")))
    assert len(fs) > 40
    return fs


def test_lazy_reading_gives_the_same_lines_on_every_golden(golden_dir, tmp_path):
    n_rec = 0
    for f in goldens(golden_dir):
        for mode in ("u", "b"):
            bcf = str(tmp_path / "g.bcf")
            subprocess.check_call([VIEW, "-O", mode, "-o", bcf, f])
            plain = subprocess.run([VIEW, bcf], check=True, stdout=subprocess.PIPE).stdout
            lazy = subprocess.run([VIEW, "--lazy", bcf], check=True, stdout=subprocess.PIPE).stdout
            assert lazy == plain, (f, mode)
            n_rec += sum(1 for ln in plain.splitlines() if not ln.startswith(b"#"))
        again = subprocess.run([VIEW, "--lazy", "-O", "u", bcf], check=True, stdout=subprocess.PIPE).stdout       # and written back as BCF
        assert again == subprocess.run([VIEW, "-O", "u", bcf], check=True, stdout=subprocess.PIPE).stdout
    assert n_rec > 5000


def test_lazy_reading_from_a_pipe_and_without_samples(golden_dir, tmp_path):
    f = os.path.join(golden_dir, "call", "mpileup.vcf")
    bcf = subprocess.run([VIEW, "-O", "u", f], check=True, stdout=subprocess.PIPE).stdout
    plain = subprocess.run([VIEW, "-"], input=bcf, check=True, stdout=subprocess.PIPE).stdout
    assert subprocess.run([VIEW, "--lazy", "-"], input=bcf, check=True, stdout=subprocess.PIPE).stdout == plain
    sites = tmp_path / "sites.vcf"                               # eight columns: nothing behind INFO
    sites.write_text("##fileformat=VCFv4.2\n##contig=<ID=1>\n##INFO=<ID=DP,Number=1,Type=Integer,Description=\"d\">\n"
                     "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n1\t5\t.\tA\tC\t3.5\t.\tDP=4\n1\t9\trs\tG\t.\t.\tPASS\t.\n")
    bcf = subprocess.run([VIEW, "-O", "u", str(sites)], check=True, stdout=subprocess.PIPE).stdout
    plain = subprocess.run([VIEW, "-H", "-"], input=bcf, check=True, stdout=subprocess.PIPE).stdout
    assert plain.count(b"\n") == 2
    assert subprocess.run([VIEW, "-H", "--lazy", "-"], input=bcf, check=True, stdout=subprocess.PIPE).stdout == plain


def test_lazy_reading_refuses_text_input(golden_dir):
    f = os.path.join(golden_dir, "call", "mpileup.vcf")
    r = subprocess.run([VIEW, "--lazy", f], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1
    assert b"can only be read from a BCF file" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if not ln.startswith(b"#")]


def test_lazy_reading_refuses_a_truncated_block(golden_dir, tmp_path):
    """The key walk checks truncation as vio_read_line does: a record whose per-sample block is cut short fails either way."""
    import struct
    f = os.path.join(golden_dir, "call", "mpileup.vcf")
    raw = bytearray(subprocess.run([VIEW, "-O", "u", f], check=True, stdout=subprocess.PIPE).stdout)
    off = 9 + struct.unpack_from("<I", raw, 5)[0]
    l_shared, l_indiv = struct.unpack_from("<II", raw, off)
    cut = raw[:off + 8 + l_shared + l_indiv - 7]
    struct.pack_into("<I", cut, off + 4, l_indiv - 7)            # a well-framed record whose last key's values run past it
    for opt in ([], ["--lazy"]):
        r = subprocess.run([VIEW] + opt + ["-"], input=bytes(cut), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1 and b"truncated BCF record" in r.stderr, opt
