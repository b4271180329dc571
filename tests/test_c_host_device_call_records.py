"""`bcfgpu_call --device-records`: with BCF output the caller's GT, PL and GQ are not downloaded as planes, printed and parsed
back -- bcfgpu_call_encode_bcf makes their BCF2 key blocks in HBM for the records that are written, the other FORMAT keys' blocks
and GP's are made on the host from their text (vio_encode_keys), and a record is its head and the blocks in the text route's
order.  The output must be the output without the option, byte for byte, and the reference's goldens, whole files: every
argument row of the `call -m` goldens on text and on BCF input with -O u and -O b, the -C alleles rows with -i, -g and -O v
(where the option does nothing), together with --device-input, the pipe from bcfgpu_sam, and a 70-sample cohort with
pass-through keys (Number=R trimming included) and without any.  --timing's extra line counts the records encoded."""
import os
import re
import subprocess

import pytest

from tests.test_c_host import CALL_EXE, SAM_EXE, VIEW_EXE, build_host, normalised
from tests.test_c_host_device_records import _cohort_sam

pytestmark = pytest.mark.gpu

OPT = "--device-records"

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
    m = re.search(rb"device records: (\d+) records' FORMAT blocks encoded on the device\n", stderr)
    assert m, stderr
    return int(m.group(1))


def as_text(bcf):
    return subprocess.run([VIEW_EXE, "-"], input=bcf, check=True, stdout=subprocess.PIPE).stdout.decode()


def n_records(text):
    return sum(1 for ln in text.splitlines() if ln and not ln.startswith("#"))


def same_with_and_without(cmd, modes=("u", "b"), extra=()):
    """cmd -O u and -O b without the option and with it (and `extra`): the same bytes on stdout.  Returns (the -O u output as
    text, the number of records whose blocks the device encoded)."""
    text, count = None, None
    for mode in modes:
        plain = subprocess.run(cmd[:1] + ["-O", mode] + cmd[1:], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        dev = subprocess.run(cmd[:1] + [OPT, "--timing", "-O", mode] + list(extra) + cmd[1:], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert plain.stderr == b""
        assert dev.stdout == plain.stdout, mode
        assert count is None or count == device_count(dev.stderr)
        count = device_count(dev.stderr)
        text = text or as_text(plain.stdout)
    return text, count


@pytest.mark.parametrize("bcf_in", [False, True], ids=["vcf-in", "bcf-in"])
@pytest.mark.parametrize("vcff,goldf,args", CALL_ROWS, ids=["%s:%s" % (r[1], r[2].replace("{G}/", "")) for r in CALL_ROWS])
def test_device_call_records_on_every_call_golden(golden_dir, tmp_path, vcff, goldf, args, bcf_in):
    build_host()
    G = os.path.join(golden_dir, "call")
    src = os.path.join(G, vcff)
    if bcf_in:
        src = to_bcf(src, str(tmp_path / "in.bcf"))
    cmd = [CALL_EXE] + args.format(G=G).split() + [src]
    text, count = same_with_and_without(cmd)
    assert normalised(text) == normalised(open(os.path.join(G, goldf)).read())
    # every record that is written was encoded on the device; -g: the option does nothing
    assert count == (0 if args == "-mg0" else n_records(text)) and n_records(text) > 0


@pytest.mark.parametrize("vcff,goldf,tab,ins", CALS_ROWS)
def test_device_call_records_with_constrained_alleles(golden_dir, vcff, goldf, tab, ins):
    """-C alleles: the records go to the device in the targets' alleles; the -i lines of targets that met no record are the
    host's (GT alone, no block of the device) and are not counted."""
    build_host()
    G = os.path.join(golden_dir, "call")
    cmd = [CALL_EXE, "-m", "-A", "-C", "alleles", "-T", os.path.join(G, tab)] + (["-i"] if ins else []) + [os.path.join(G, vcff)]
    text, count = same_with_and_without(cmd, modes=("u",))
    assert normalised(text) == normalised(open(os.path.join(G, goldf)).read())
    missed = sum(1 for ln in text.splitlines() if not ln.startswith("#") and ln.split("\t")[8] == "GT")
    assert count == n_records(text) - missed > 0 and (ins or missed == 0)


def test_the_option_does_nothing_with_text_output_and_with_gvcf(golden_dir):
    build_host()
    G = os.path.join(golden_dir, "call")
    vcf = os.path.join(G, "mpileup.vcf")
    for args, mode in (("-v", "v"), ("-v", "z"), ("-mg0", "u"), ("-mg0", "v")):
        plain = subprocess.run([CALL_EXE, "-O", mode] + args.split() + [vcf], check=True, stdout=subprocess.PIPE).stdout
        dev = subprocess.run([CALL_EXE, OPT, "--timing", "-O", mode] + args.split() + [vcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert dev.stdout == plain and device_count(dev.stderr) == 0
    assert normalised(plain.decode()) == normalised(open(os.path.join(G, "mpileup.2.out")).read())


def test_timing_line_and_a_silent_stderr(golden_dir, tmp_path):
    """--timing: the two lines there were, unchanged, and the new one; without --timing nothing on stderr."""
    build_host()
    G = os.path.join(golden_dir, "call")
    bcf = to_bcf(os.path.join(G, "mpileup.vcf"), str(tmp_path / "in.bcf"))
    quiet = subprocess.run([CALL_EXE, OPT, "-v", "-O", "u", bcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    timed = subprocess.run([CALL_EXE, OPT, "--timing", "-v", "-O", "u", bcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    off = subprocess.run([CALL_EXE, "--timing", "-v", "-O", "u", bcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert quiet.stderr == b"" and quiet.stdout == timed.stdout == off.stdout
    assert device_count(timed.stderr) == n_records(as_text(timed.stdout)) == 11 and device_count(off.stderr) == 0
    for err in (timed.stderr, off.stderr):
        assert re.search(rb"seconds: reading records [\d.]+, building the planes on the host [\d.]+, uploads and device stages [\d.]+, writing records [\d.]+\n", err)
        assert re.search(rb"device input: 0 records' planes decoded on the device\n", err)
        assert err.count(b"\n") == 3


@pytest.mark.parametrize("vcff,goldf,args", [CALL_ROWS[0], CALL_ROWS[6], CALL_ROWS[13], CALL_ROWS[19]], ids=lambda x: None)
def test_device_call_records_together_with_device_input(golden_dir, tmp_path, vcff, goldf, args):
    build_host()
    G = os.path.join(golden_dir, "call")
    bcf = to_bcf(os.path.join(G, vcff), str(tmp_path / "in.bcf"))
    cmd = [CALL_EXE] + args.format(G=G).split() + [bcf]
    text, count = same_with_and_without(cmd, modes=("u",), extra=["--device-input"])
    assert normalised(text) == normalised(open(os.path.join(G, goldf)).read()) and count == n_records(text) > 0


def test_device_call_records_from_the_pipe(golden_dir, tmp_path):
    """`bcfgpu_sam -O u ... | bcfgpu_call --device-input --device-records -v -O u -` against the same through a file, option off."""
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    sam_cmd = [SAM_EXE, "-O", "u", os.path.join(G, "mpileup.ref.fa"), "17", "100", "600"] + [os.path.join(G, "mpileup.%d.sam" % i) for i in (1, 2, 3)]
    bcf = str(tmp_path / "m.bcf")
    with open(bcf, "wb") as f:
        subprocess.run(sam_cmd, check=True, stdout=f)
    via_file = subprocess.run([CALL_EXE, "-v", "-O", "u", bcf], check=True, stdout=subprocess.PIPE).stdout
    for extra in ([], ["--device-input"]):
        p1 = subprocess.Popen(sam_cmd, stdout=subprocess.PIPE)
        via_pipe = subprocess.run([CALL_EXE, OPT, "--timing", "-v", "-O", "u"] + extra + ["-"], stdin=p1.stdout, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        p1.stdout.close()
        assert p1.wait() == 0
        assert via_pipe.stdout == via_file
        assert device_count(via_pipe.stderr) == n_records(as_text(via_file)) >= 1


@pytest.fixture(scope="module")
def cohort(golden_dir, tmp_path_factory):
    """70 single-sample files over 200 columns through `bcfgpu_sam -O u`, with -a AD,DP (pass-through keys, AD is Number=R)
    and with the default FORMAT (PL alone): more samples than a wavefront has lanes."""
    build_host()
    d = tmp_path_factory.mktemp("cohort")
    G = os.path.join(golden_dir, "mpileup")
    ref = "".join(ln.strip() for ln in open(os.path.join(G, "mpileup.ref.fa")) if not ln.startswith(">"))
    files = []
    for s in range(70):
        files.append(str(d / ("c%02d.sam" % s)))
        _cohort_sam(files[-1], ref, "c%02d" % s, 1000 + s, 1000, 1200)
    tail = ["-f", os.path.join(G, "mpileup.ref.fa"), "-r", "17:1001-1200"] + files
    subprocess.check_call([SAM_EXE, "-a", "AD,DP", "-O", "u", "-o", str(d / "ad.bcf")] + tail)
    subprocess.check_call([SAM_EXE, "-O", "u", "-o", str(d / "plain.bcf")] + tail)
    names = ["c%02d" % s for s in range(70)]
    (d / "reversed.txt").write_text("".join(n + "\n" for n in names[::-1]))
    (d / "three.txt").write_text("c41\nc03\nc69\n")
    (d / "groups.txt").write_text("".join("%s\t%s\n" % (n, "even" if i % 2 == 0 else "odd") for i, n in enumerate(names)))
    return d


@pytest.mark.parametrize("dev_in", [False, True], ids=["", "device-input"])
@pytest.mark.parametrize("src,args,n_smpl", [("ad", "-v", 70), ("ad", "", 70), ("ad", "-v -S {D}/reversed.txt", 70), ("ad", "-S {D}/three.txt", 3),
                                             ("ad", "-v -G {D}/groups.txt --group-samples-tag AD", 70), ("ad", "--ploidy 1", 70),
                                             ("ad", "-v -a GQ,GP", 70), ("plain", "-v", 70), ("plain", "", 70), ("plain", "-v -a GQ", 70)])
def test_device_call_records_on_a_cohort_past_one_wavefront(cohort, src, args, n_smpl, dev_in):
    d = cohort
    cmd = [CALL_EXE] + args.format(D=str(d)).split() + [str(d / (src + ".bcf"))]
    text, count = same_with_and_without(cmd, modes=("u",), extra=["--device-input"] if dev_in else [])
    recs = [ln.split("\t") for ln in text.splitlines() if not ln.startswith("#")]
    assert count == len(recs) > 0 and all(len(r) == 9 + n_smpl for r in recs)
    assert len(recs) >= 200 or "-v" in args
    fmts = {r[8] for r in recs}
    if src == "ad":
        assert all(f.startswith("GT:PL:DP:AD") or f.startswith("GT:DP:AD") for f in fmts), fmts
        for r in recs:                                           # alleles were dropped: AD (Number=R) follows them
            assert len(r[9].split(":")[r[8].split(":").index("AD")].split(",")) == 1 + (0 if r[4] == "." else len(r[4].split(","))), r[:10]
    else:
        assert fmts <= {"GT:PL", "GT", "GT:PL:GQ"}, fmts
    if "--ploidy" in args:
        assert all("/" not in c.split(":")[0] for r in recs for c in r[9:])
    if "GQ,GP" in args:
        assert any(f.endswith(":GP:GQ") for f in fmts)
