"""`bcfgpu_call --device-text`: with -O v|z and --device-input in effect the sample columns of the written records are formatted on the
device (bcfgpu_call_encode_vcf: GT, the input's keys in their order with the trimmed PL in PL's place, GQ) and the host prints the
head alone; a record with GP or with a key that is not stored as integers stays on the host.  The output must be the output without
any option, byte for byte, and the reference's goldens: every argument row of the `call -m` goldens on BCF input with -O v and -O z,
a 70-sample cohort with five pass-through keys, a record with a Float key, the runs in which the option does nothing, and the pipe
from bcfgpu_sam.  --timing's extra line counts the records formatted on the device and on the host."""
import gzip
import os
import re
import subprocess

import pytest

from tests.test_c_host import CALL_EXE, SAM_EXE, VIEW_EXE, build_host, normalised
from tests.test_c_host_device_call_records import CALL_ROWS, n_records, to_bcf
from tests.test_c_host_device_keys import COHORT_KEYS, cohort  # noqa: F401  (the 70-sample fixture)

pytestmark = pytest.mark.gpu

OPTS = ["--device-input", "--device-text"]
EVERY = ["--device-input", "--device-records", "--device-keys", "--device-text"]


def text_counts(stderr, lines=4):
    """(N, M) of the --device-text line; the lines that were there are still there, in their order, and nothing else."""
    got = stderr.split(b"\n")
    assert len(got) == lines + 1 and got[-1] == b"", stderr
    assert got[0].startswith(b"[bcfgpu_call] seconds: reading records ") and got[1].startswith(b"[bcfgpu_call] device input: ")
    assert got[2].startswith(b"[bcfgpu_call] device records: ")
    m = re.fullmatch(rb"\[bcfgpu_call\] device text: (\d+) records' sample columns formatted on the device, (\d+) on the host", got[-2])
    assert m, stderr
    return int(m.group(1)), int(m.group(2))


def same_with_and_without(cmd, modes=("v", "z"), opts=OPTS, lines=4):
    """cmd -O v and -O z without any option and with `opts`: the same bytes on stdout.  Returns (the -O v output as text, (N, M))."""
    text = counts = None
    for mode in modes:
        plain = subprocess.run(cmd[:1] + ["-O", mode] + cmd[1:], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        dev = subprocess.run(cmd[:1] + list(opts) + ["--timing", "-O", mode] + cmd[1:], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert plain.stderr == b""
        assert dev.stdout == plain.stdout, mode
        assert counts is None or counts == text_counts(dev.stderr, lines)
        counts = text_counts(dev.stderr, lines)
        text = text or (plain.stdout if mode == "v" else gzip.decompress(plain.stdout)).decode()
    return text, counts


def records(text):
    return [ln.split("\t") for ln in text.splitlines() if ln and not ln.startswith("#")]


@pytest.mark.parametrize("vcff,goldf,args", CALL_ROWS, ids=["%s:%s" % (r[1], r[2].replace("{G}/", "")) for r in CALL_ROWS])
def test_device_text_on_every_call_golden(golden_dir, tmp_path, vcff, goldf, args):
    build_host()
    G = os.path.join(golden_dir, "call")
    bcf = to_bcf(os.path.join(G, vcff), str(tmp_path / "in.bcf"))
    cmd = [CALL_EXE] + args.format(G=G).split() + [bcf]
    text, (n_dev, n_host) = same_with_and_without(cmd)
    assert normalised(text) == normalised(open(os.path.join(G, goldf)).read()) and n_records(text) > 0
    if args == "-mg0":                                          # -g: the option does nothing
        assert n_dev == 0
    else:
        recs = records(text)
        assert n_dev + n_host == len(recs)
        assert n_host == sum("GP" in r[8].split(":") for r in recs)
        assert n_dev > 0 or "GP" in args


@pytest.mark.parametrize("args,n_smpl", [("-v", 70), ("", 70), ("-v -S {D}/reversed.txt", 70), ("-S {D}/three.txt", 3),
                                         ("-v -G {D}/groups.txt --group-samples-tag AD", 70), ("--ploidy 1", 70), ("-v -a GQ,GP", 70), ("-a GQ,GP", 70)])
def test_device_text_on_a_cohort_past_one_wavefront(cohort, args, n_smpl):  # noqa: F811
    d = cohort
    cmd = [CALL_EXE] + args.format(D=str(d)).split() + [str(d / "keys.bcf")]
    text, (n_dev, n_host) = same_with_and_without(cmd, modes=("v",))
    recs = records(text)
    assert n_dev + n_host == len(recs) > 0 and all(len(r) == 9 + n_smpl for r in recs)
    assert len(recs) >= 200 or "-v" in args
    assert all(set(COHORT_KEYS) <= set(r[8].split(":")) for r in recs)
    if "GP" in args:
        # a called variant record carries GP and is the host's.  Under -v every written record is one, so the device formats none;
        # without -v the reference records beside them are the device's: both routes in one run
        assert n_host == sum("GP" in r[8].split(":") for r in recs) > 0
        assert n_dev == (0 if "-v" in args else sum("GP" not in r[8].split(":") for r in recs)) and ("-v" in args or n_dev > 0)
    else:
        assert n_host == 0
    for r in recs:                                                  # alleles were dropped: the Number=R keys follow them
        keys = r[8].split(":")
        for k in ("AD", "ADF", "ADR"):
            assert len(r[9].split(":")[keys.index(k)].split(",")) == 1 + (0 if r[4] == "." else len(r[4].split(","))), r[:10]


FLOAT_VCF = """##fileformat=VCFv4.2
##FILTER=<ID=PASS,Description="All filters passed">
##contig=<ID=1,length=1000>
##INFO=<ID=QS,Number=R,Type=Float,Description="x">
##INFO=<ID=I16,Number=16,Type=Float,Description="x">
##FORMAT=<ID=PL,Number=G,Type=Integer,Description="x">
##FORMAT=<ID=AD,Number=R,Type=Integer,Description="x">
##FORMAT=<ID=XF,Number=1,Type=Float,Description="x">
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb
1\t10\t.\tA\tC,<*>\t0\t.\tQS=1,1,0;I16=10,10,10,10,600,18000,600,18000,1200,36000,1200,36000,400,8000,400,8000\tPL:AD:XF\t0,30,200,30,200,200:10,0,0:0.5\t200,30,0,200,30,200:0,10,0:1.25
1\t20\t.\tG\tT,<*>\t0\t.\tQS=1,1,0;I16=10,10,10,10,600,18000,600,18000,1200,36000,1200,36000,400,8000,400,8000\tPL:AD\t0,30,200,30,200,200:10,0,0\t200,30,0,200,30,200:0,10,0
"""


def test_a_record_with_a_float_key_stays_on_the_host(tmp_path):
    build_host()
    bcf = str(tmp_path / "float.bcf")
    with open(bcf, "wb") as f:
        subprocess.run([VIEW_EXE, "-O", "u", "-"], input=FLOAT_VCF.encode(), check=True, stdout=f)
    text, counts = same_with_and_without([CALL_EXE, bcf])
    recs = records(text)
    assert len(recs) == 2 and recs[0][8] == "GT:PL:AD:XF" and recs[1][8] == "GT:PL:AD" and counts == (1, 1)
    assert recs[0][9].endswith(":0.5") and (recs[0][4], recs[1][4]) == ("C", "T") and recs[1][9].split(":")[2] == "10,0"


NOTHING = [("text-input", "-v {vcf}", "v", OPTS), ("bcf-output", "-v {bcf}", "u", OPTS), ("gvcf", "-g 0 {bcf}", "v", OPTS),
           ("constrained-alleles", "-m -A -C alleles -T {G}/mpileup.tab {bcf}", "v", OPTS), ("without-device-input", "-v {bcf}", "v", OPTS[1:]),
           ("every-option-bcf-output", "-v {bcf}", "u", EVERY)]


@pytest.mark.parametrize("tail,mode,opts", [r[1:] for r in NOTHING], ids=[r[0] for r in NOTHING])
def test_the_option_does_nothing_where_it_should(golden_dir, tmp_path, tail, mode, opts):
    """Text input, -O u, -g, -C alleles and the option without --device-input: the same bytes and no record formatted on the device."""
    build_host()
    G = os.path.join(golden_dir, "call")
    vcf = os.path.join(G, "mpileup.vcf" if "alleles" in tail else "mpileup.hwe.vcf")
    tail = tail.format(G=G, vcf=vcf, bcf=to_bcf(vcf, str(tmp_path / "in.bcf")) if "{bcf}" in tail else None).split()
    plain = subprocess.run([CALL_EXE, "-O", mode] + tail, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    dev = subprocess.run([CALL_EXE] + opts + ["--timing", "-O", mode] + tail, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert plain.stderr == b"" and dev.stdout == plain.stdout and len(plain.stdout) > 0
    assert text_counts(dev.stderr, 5 if opts is EVERY else 4)[0] == 0


def test_every_option_together_acts_on_its_own_output_mode(golden_dir, tmp_path):
    """--device-records and --device-keys given beside --device-text: with -O v the text option alone acts."""
    build_host()
    G = os.path.join(golden_dir, "call")
    bcf = to_bcf(os.path.join(G, "mpileup.hwe.vcf"), str(tmp_path / "in.bcf"))
    text, (n_dev, n_host) = same_with_and_without([CALL_EXE, "-v", bcf], opts=EVERY, lines=5)
    assert n_dev == n_records(text) > 0 and n_host == 0


def test_stderr_without_the_option_and_without_timing(golden_dir, tmp_path):
    """Without --device-text --timing prints exactly the lines it printed before; without --timing nothing is printed."""
    build_host()
    G = os.path.join(golden_dir, "call")
    bcf = to_bcf(os.path.join(G, "mpileup.hwe.vcf"), str(tmp_path / "in.bcf"))
    base = [CALL_EXE, "-v", "-O", "v"]
    quiet = subprocess.run(base + OPTS + [bcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    off = subprocess.run(base + OPTS[:1] + ["--timing", bcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    on = subprocess.run(base + OPTS + ["--timing", bcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert quiet.stderr == b"" and quiet.stdout == off.stdout == on.stdout
    lines = off.stderr.split(b"\n")
    assert len(lines) == 4 and lines[3] == b"" and b"device text" not in off.stderr
    assert lines[0].startswith(b"[bcfgpu_call] seconds: reading records ") and lines[1].startswith(b"[bcfgpu_call] device input: ")
    assert lines[2].startswith(b"[bcfgpu_call] device records: ")
    assert [re.sub(rb"[\d.]+", b"#", x) for x in on.stderr.split(b"\n")[:3]] == [re.sub(rb"[\d.]+", b"#", x) for x in lines[:3]]
    assert text_counts(on.stderr)[0] > 0


def test_device_text_from_the_pipe(golden_dir, tmp_path):
    """`bcfgpu_sam -a AD,DP -O u ... | bcfgpu_call --device-input --device-text -v -O v -` against the same through a file with no
    option."""
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    sam_cmd = [SAM_EXE, "-a", "AD,DP", "-O", "u", "-f", os.path.join(G, "mpileup.ref.fa"), "-r", "17:100-600"] + [os.path.join(G, "mpileup.%d.sam" % i) for i in (1, 2, 3)]
    bcf = str(tmp_path / "m.bcf")
    with open(bcf, "wb") as f:
        subprocess.run(sam_cmd, check=True, stdout=f)
    via_file = subprocess.run([CALL_EXE, "-v", "-O", "v", bcf], check=True, stdout=subprocess.PIPE).stdout
    p1 = subprocess.Popen(sam_cmd, stdout=subprocess.PIPE)
    via_pipe = subprocess.run([CALL_EXE] + OPTS + ["--timing", "-v", "-O", "v", "-"], stdin=p1.stdout, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    p1.stdout.close()
    assert p1.wait() == 0
    assert via_pipe.stdout == via_file
    n = n_records(via_file.decode())
    assert text_counts(via_pipe.stderr) == (n, 0) and n >= 1
