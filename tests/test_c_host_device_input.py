"""`bcfgpu_call --device-input`: BCF input does not go through text -- the records' per-sample blocks go to the device as the
file holds them, bcfgpu_call_decode_bcf makes the PL (and AD) planes there, and the sample columns become text only for the
records that are written.  The output must be the output without the option, byte for byte, and the reference's goldens,
whole files: every argument row of the `call -m` goldens on the input turned into BCF (-O u and -O b), the -C alleles rows
and -g (where the option does nothing), text input (likewise), the pipe from bcfgpu_sam, and a 70-sample cohort with -S, -G,
--ploidy and -a.  --timing's extra line tells how many records' planes were decoded on the device."""
import os
import re
import subprocess

import pytest

from tests.test_c_host import CALL_EXE, SAM_EXE, VIEW_EXE, build_host, normalised, whole_file_checks
from tests.test_c_host_device_records import _cohort_sam

pytestmark = pytest.mark.gpu

OPT = "--device-input"

# the argument rows of tests/test_c_host.py::test_c_call_driver_reproduces_reference_golden, restated
CALL_ROWS = [
    ("mpileup.vcf", "mpileup.1.out", "-v"), ("mpileup.vcf", "mpileup.3.out", "-v -S {G}/mpileup.3.samples"),
    ("mpileup.vcf", "mpileup.3.out", "-v -s HG00100,HG00101,HG00102 -p 0.5 --threads 2"),
    ("mpileup.vcf", "mpileup.3.out", "--multiallelic-caller --variants-only --samples-file {G}/mpileup.3.samples"),
    ("mpileup.vcf", "mpileup.4.out", "-v -S {G}/mpileup.4.samples"), ("mpileup.vcf", "mpileup.5.out", "-v -S {G}/mpileup.5.samples"),
    ("mpileup.X.vcf", "mpileup.X.out", "-v -S {G}/mpileup.samples --ploidy-file {G}/mpileup.ploidy"),
    ("mpileup.X.vcf", "mpileup.X.out", "-v -S {G}/mpileup.ped --ploidy-file {G}/mpileup.ploidy"),
    ("mpileup.X.vcf", "mpileup.X.2.out", "-v -S {G}/mpileup.2.samples --ploidy-file {G}/mpileup.ploidy"),
    ("mpileup.NA19213.NA19129.vcf", "mpileup.hwe.1.out", "-v"), ("mpileup.hwe.vcf", "mpileup.hwe.2.out", "-v"),
    ("mpileup.NA19213.NA19129.vcf", "mpileup.hwe.1b.out", "-v -G - --group-samples-tag AD"),
    ("mpileup.hwe.vcf", "mpileup.hwe.3.out", "-v -G - --group-samples-tag AD"),
    ("mpileup.hwe.vcf", "mpileup.hwe.4.out", "-v -G {G}/mpileup.hwe.samples --group-samples-tag AD"),
    ("call-G.vcf", "call-G.1.out", "-v"), ("call-G.vcf", "call-G.2.out", "-v -G - --group-samples-tag AD"),
    ("call-G.2.vcf", "call-G.2.1.out", "-v -F AN_POP,AC_POP"),
    ("call.af-fixation.vcf", "call.af-fixation.1.out", ""),
    ("call.af-fixation.vcf", "call.af-fixation.2.out", "-G {G}/call.af-fixation.txt"),
    ("call.af-fixation.vcf", "call.af-fixation.3.out", "-G {G}/call.af-fixation.txt -a GP,GQ"),
    ("mpileup.vcf", "mpileup.2.out", "-mg0"),
]
# ... and of test_c_call_driver_constrained_alleles
CALS_ROWS = [
    ("mpileup.vcf", "mpileup.cAls.out", "mpileup.tab", False), ("mpileup.2.vcf", "mpileup.cAls.2.out", "mpileup.2.tab", False),
    ("mpileup.3.vcf", "mpileup.cAls.3.out", "mpileup.3.tab", True), ("mpileup.3.vcf", "mpileup.cAls.4.out", "mpileup.4.tab", True),
    ("mpileup.3.vcf", "mpileup.cAls.5.out", "mpileup.5.tab", True), ("mpileup.4.vcf", "mpileup.cAls.6.out", "mpileup.6.tab", True),
    ("mpileup.5.vcf", "mpileup.cAls.7.out", "mpileup.7.tab", True),
    ("mpileup.cals.1.vcf", "mpileup.cals.8.out", "mpileup.cals.1.tab", False),
    ("mpileup.cals.2.vcf", "mpileup.cals.9.out", "mpileup.cals.2.tab", False),
]


def to_bcf(vcf, path, mode="u"):
    subprocess.check_call([VIEW_EXE, "-O", mode, "-o", path, vcf])
    return path


def device_count(stderr):
    assert b"reading records" in stderr and b"writing records" in stderr
    m = re.search(rb"device input: (\d+) records' planes decoded on the device", stderr)
    assert m, stderr
    return int(m.group(1))


def same_with_and_without(cmd, modes=("v", "u")):
    """cmd -O v and -O u with and without the option: the same bytes on stdout.  Returns (the -O v bytes, the number of records
    whose planes the device decoded)."""
    text, count = None, None
    for mode in modes:
        plain = subprocess.run(cmd[:1] + ["-O", mode] + cmd[1:], check=True, stdout=subprocess.PIPE).stdout
        dev = subprocess.run(cmd[:1] + [OPT, "--timing", "-O", mode] + cmd[1:], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert dev.stdout == plain, mode
        assert count is None or count == device_count(dev.stderr)
        count = device_count(dev.stderr)
        text = text or plain
    return text, count


def kept_records(vcf):
    """The records `call` keeps of an input: all but those whose reference allele starts with N (vcfcall.c:1095-1099)."""
    return sum(1 for ln in open(vcf) if not ln.startswith("#") and ln.strip() and ln.split("\t")[3][0] not in "Nn")


@pytest.mark.parametrize("mode", ["u", "b"])
@pytest.mark.parametrize("vcff,goldf,args", CALL_ROWS, ids=["%s:%s" % (r[1], r[2].replace("{G}/", "")) for r in CALL_ROWS])
def test_device_input_on_every_call_golden(golden_dir, tmp_path, vcff, goldf, args, mode):
    build_host()
    G = os.path.join(golden_dir, "call")
    bcf = to_bcf(os.path.join(G, vcff), str(tmp_path / "in.bcf"), mode)
    cmd = [CALL_EXE] + args.format(G=G).split() + [bcf]
    whole_file_checks(cmd[:1] + [OPT] + cmd[1:], os.path.join(G, goldf))
    text, count = same_with_and_without(cmd)
    assert sum(1 for ln in text.splitlines() if not ln.startswith(b"#")) > 0
    assert count == (0 if args == "-mg0" else kept_records(os.path.join(G, vcff))) and (count > 0 or args == "-mg0")


@pytest.mark.parametrize("vcff,goldf,tab,ins", CALS_ROWS)
def test_device_input_does_nothing_with_constrained_alleles(golden_dir, tmp_path, vcff, goldf, tab, ins):
    build_host()
    G = os.path.join(golden_dir, "call")
    bcf = to_bcf(os.path.join(G, vcff), str(tmp_path / "in.bcf"))
    cmd = [CALL_EXE, "-m", "-A", "-C", "alleles", "-T", os.path.join(G, tab)] + (["-i"] if ins else []) + [bcf]
    text, count = same_with_and_without(cmd, modes=("v",))
    assert count == 0
    assert normalised(text.decode()) == normalised(open(os.path.join(G, goldf)).read())


def test_device_input_does_nothing_on_text_input(golden_dir):
    build_host()
    G = os.path.join(golden_dir, "call")
    text, count = same_with_and_without([CALL_EXE, "-v", os.path.join(G, "mpileup.vcf")])
    assert count == 0
    assert normalised(text.decode()) == normalised(open(os.path.join(G, "mpileup.1.out")).read())


def test_timing_alone_changes_nothing_on_stdout(golden_dir, tmp_path):
    build_host()
    G = os.path.join(golden_dir, "call")
    bcf = to_bcf(os.path.join(G, "mpileup.vcf"), str(tmp_path / "in.bcf"))
    plain = subprocess.run([CALL_EXE, "-v", bcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    timed = subprocess.run([CALL_EXE, "-v", "--timing", bcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert timed.stdout == plain.stdout and plain.stderr == b"" and device_count(timed.stderr) == 0
    assert re.search(rb"seconds: reading records [\d.]+, building the planes on the host [\d.]+, uploads and device stages [\d.]+, writing records [\d.]+\n", timed.stderr)


def test_device_input_from_the_pipe(golden_dir, tmp_path):
    """`bcfgpu_sam -O u ... | bcfgpu_call --device-input -v -` against the same through a file."""
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    sam_cmd = [SAM_EXE, "-O", "u", os.path.join(G, "mpileup.ref.fa"), "17", "100", "600"] + [os.path.join(G, "mpileup.%d.sam" % i) for i in (1, 2, 3)]
    bcf = str(tmp_path / "m.bcf")
    with open(bcf, "wb") as f:
        subprocess.run(sam_cmd, check=True, stdout=f)
    via_file = subprocess.run([CALL_EXE, "-v", bcf], check=True, stdout=subprocess.PIPE).stdout
    p1 = subprocess.Popen(sam_cmd, stdout=subprocess.PIPE)
    via_pipe = subprocess.run([CALL_EXE, OPT, "--timing", "-v", "-"], stdin=p1.stdout, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p1.wait() == 0
    assert via_pipe.stdout == via_file
    assert device_count(via_pipe.stderr) > 400
    assert sum(1 for ln in via_file.splitlines() if not ln.startswith(b"#")) >= 1


@pytest.fixture(scope="module")
def cohort(golden_dir, tmp_path_factory):
    """70 single-sample files over 200 columns through `bcfgpu_sam -a AD,DP -O u`: more samples than a wavefront has lanes."""
    build_host()
    d = tmp_path_factory.mktemp("cohort")
    G = os.path.join(golden_dir, "mpileup")
    ref = "".join(ln.strip() for ln in open(os.path.join(G, "mpileup.ref.fa")) if not ln.startswith(">"))
    files = []
    for s in range(70):
        files.append(str(d / ("c%02d.sam" % s)))
        _cohort_sam(files[-1], ref, "c%02d" % s, 1000 + s, 1000, 1200)
    bcf = str(d / "cohort.bcf")
    subprocess.check_call([SAM_EXE, "-a", "AD,DP", "-O", "u", "-o", bcf, "-f", os.path.join(G, "mpileup.ref.fa"), "-r", "17:1001-1200"] + files)
    names = ["c%02d" % s for s in range(70)]
    (d / "reversed.txt").write_text("".join(n + "\n" for n in names[::-1]))
    (d / "three.txt").write_text("c41\nc03\nc69\n")
    (d / "groups.txt").write_text("".join("%s\t%s\n" % (n, "even" if i % 2 == 0 else "odd") for i, n in enumerate(names)))
    return d, bcf


@pytest.mark.parametrize("args,n_smpl", [("-v", 70), ("", 70), ("-v -S {D}/reversed.txt", 70), ("-S {D}/three.txt", 3),
                                         ("-v -G {D}/groups.txt --group-samples-tag AD", 70), ("--ploidy 1", 70), ("-v -a GQ,GP", 70)])
def test_device_input_on_a_cohort_past_one_wavefront(cohort, args, n_smpl):
    d, bcf = cohort
    cmd = [CALL_EXE] + args.format(D=str(d)).split() + [bcf]
    text, count = same_with_and_without(cmd)
    recs = [ln.split(b"\t") for ln in text.splitlines() if not ln.startswith(b"#")]
    assert count >= 200 and 0 < len(recs) <= count and all(len(r) == 9 + n_smpl for r in recs)
    assert len(recs) < count or "-v" not in args
    if "--ploidy" in args:                                       # haploid genotypes (no variant of this cohort survives haploid calling, also with the prior counting 70 alleles, not 140: every record is kept instead)
        assert all(b"/" not in c.split(b":")[0] for r in recs for c in r[9:])
    if "GQ" in args:
        assert any(r[8].endswith(b":GP:GQ") for r in recs)
    if "reversed" in args:
        hdr = [ln for ln in text.splitlines() if ln.startswith(b"#CHROM")][0].split(b"\t")
        assert hdr[9] == b"c69" and hdr[-1] == b"c00"
