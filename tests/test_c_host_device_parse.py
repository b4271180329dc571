"""`bcfgpu_call --device-parse`: VCF text input is not split and parsed on the host -- a line is cut at its ninth tab, the sample
columns go to the device as text, bcfgpu_call_decode_vcf makes the PL (and AD / QS) planes there, and a record's columns are
split on the host only when the record is written.  The output must be the output without the option, byte for byte, and the
reference's goldens, whole files: every argument row of the `call -m` goldens on the .vcf itself, one file bgzipped and on
stdin, the -C alleles rows, -g and BCF input (where the option does nothing), and a 70-sample cohort written as text with -S,
-G, --ploidy, -a and --device-records.  --timing's extra line tells how many records' planes were parsed on the device."""
import os
import re
import subprocess

import pytest

from tests.test_c_host import CALL_EXE, SAM_EXE, VIEW_EXE, build_host, normalised, whole_file_checks
from tests.test_c_host_device_input import CALL_ROWS, CALS_ROWS, device_count, kept_records, to_bcf
from tests.test_c_host_device_records import _cohort_sam

pytestmark = pytest.mark.gpu

OPT = "--device-parse"


def parse_count(stderr):
    assert b"reading records" in stderr and b"writing records" in stderr
    m = re.search(rb"device parse: (\d+) records' planes parsed on the device", stderr)
    assert m, stderr
    return int(m.group(1))


def same_with_and_without(cmd, modes=("v", "u"), stdin=None, extra=()):
    """cmd -O v and -O u with and without the option: the same bytes on stdout.  Returns (the -O v bytes, the number of records
    whose planes the device parsed)."""
    text, count = None, None
    for mode in modes:
        plain = subprocess.run(cmd[:1] + ["-O", mode] + cmd[1:], check=True, input=stdin, stdout=subprocess.PIPE).stdout
        dev = subprocess.run(cmd[:1] + [OPT, "--timing", "-O", mode] + list(extra) + cmd[1:], check=True, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert dev.stdout == plain, mode
        assert count is None or count == parse_count(dev.stderr)
        count = parse_count(dev.stderr)
        text = text or plain
    return text, count


@pytest.mark.parametrize("vcff,goldf,args", CALL_ROWS, ids=["%s:%s" % (r[1], r[2].replace("{G}/", "")) for r in CALL_ROWS])
def test_device_parse_on_every_call_golden(golden_dir, vcff, goldf, args):
    build_host()
    G = os.path.join(golden_dir, "call")
    vcf = os.path.join(G, vcff)
    cmd = [CALL_EXE] + args.format(G=G).split() + [vcf]
    whole_file_checks(cmd[:1] + [OPT] + cmd[1:], os.path.join(G, goldf))
    text, count = same_with_and_without(cmd)
    assert sum(1 for ln in text.splitlines() if not ln.startswith(b"#")) > 0
    assert count == (0 if args == "-mg0" else kept_records(vcf)) and (count > 0 or args == "-mg0")


def test_device_parse_on_bgzipped_input_and_stdin(golden_dir, tmp_path):
    build_host()
    G = os.path.join(golden_dir, "call")
    vcf = os.path.join(G, "mpileup.vcf")
    gz = str(tmp_path / "in.vcf.gz")
    subprocess.check_call([VIEW_EXE, "-O", "z", "-o", gz, vcf])
    assert open(gz, "rb").read(2) == b"\x1f\x8b"
    want = normalised(open(os.path.join(G, "mpileup.1.out")).read())
    text, count = same_with_and_without([CALL_EXE, "-v", gz])
    assert count == kept_records(vcf) and normalised(text.decode()) == want
    for data in (open(vcf, "rb").read(), open(gz, "rb").read()):
        text, count = same_with_and_without([CALL_EXE, "-v", "-"], stdin=data)
        assert count == kept_records(vcf) and normalised(text.decode()) == want


@pytest.mark.parametrize("vcff,goldf,tab,ins", CALS_ROWS)
def test_device_parse_does_nothing_with_constrained_alleles(golden_dir, vcff, goldf, tab, ins):
    build_host()
    G = os.path.join(golden_dir, "call")
    cmd = [CALL_EXE, "-m", "-A", "-C", "alleles", "-T", os.path.join(G, tab)] + (["-i"] if ins else []) + [os.path.join(G, vcff)]
    text, count = same_with_and_without(cmd, modes=("v",))
    assert count == 0
    assert normalised(text.decode()) == normalised(open(os.path.join(G, goldf)).read())


def test_device_parse_does_nothing_with_gvcf_blocks_and_on_bcf_input(golden_dir, tmp_path):
    build_host()
    G = os.path.join(golden_dir, "call")
    vcf = os.path.join(G, "mpileup.vcf")
    text, count = same_with_and_without([CALL_EXE, "-g", "0,2,5", vcf])
    assert count == 0 and sum(1 for ln in text.splitlines() if not ln.startswith(b"#")) > 0
    bcf = to_bcf(vcf, str(tmp_path / "in.bcf"))
    text, count = same_with_and_without([CALL_EXE, "-v", bcf])
    assert count == 0 and normalised(text.decode()) == normalised(open(os.path.join(G, "mpileup.1.out")).read())
    # --device-input beside it still decodes every record of BCF input; on text input it is --device-parse that acts
    both = subprocess.run([CALL_EXE, OPT, "--device-input", "--timing", "-v", bcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert both.stdout == text and parse_count(both.stderr) == 0 and device_count(both.stderr) == kept_records(vcf)
    both = subprocess.run([CALL_EXE, OPT, "--device-input", "--timing", "-v", vcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert both.stdout == text and parse_count(both.stderr) == kept_records(vcf) and device_count(both.stderr) == 0


@pytest.fixture(scope="module")
def cohort(golden_dir, tmp_path_factory):
    """70 single-sample files over 200 columns through `bcfgpu_sam -a AD,DP -O v`: more samples than a wavefront has lanes."""
    build_host()
    d = tmp_path_factory.mktemp("cohort")
    G = os.path.join(golden_dir, "mpileup")
    ref = "".join(ln.strip() for ln in open(os.path.join(G, "mpileup.ref.fa")) if not ln.startswith(">"))
    files = []
    for s in range(70):
        files.append(str(d / ("c%02d.sam" % s)))
        _cohort_sam(files[-1], ref, "c%02d" % s, 1000 + s, 1000, 1200)
    vcf = str(d / "cohort.vcf")
    subprocess.check_call([SAM_EXE, "-a", "AD,DP", "-O", "v", "-o", vcf, "-f", os.path.join(G, "mpileup.ref.fa"), "-r", "17:1001-1200"] + files)
    assert open(vcf, "rb").read(2) == b"##"
    names = ["c%02d" % s for s in range(70)]
    (d / "reversed.txt").write_text("".join(n + "\n" for n in names[::-1]))
    (d / "three.txt").write_text("c41\nc03\nc69\n")
    (d / "groups.txt").write_text("".join("%s\t%s\n" % (n, "even" if i % 2 == 0 else "odd") for i, n in enumerate(names)))
    return d, vcf


@pytest.mark.parametrize("args,n_smpl,extra", [("-v", 70, ()), ("", 70, ()), ("-v -S {D}/reversed.txt", 70, ()), ("-S {D}/three.txt", 3, ()),
                                               ("-v -G {D}/groups.txt --group-samples-tag AD", 70, ()), ("--ploidy 1", 70, ()), ("-v -a GQ,GP", 70, ()),
                                               ("", 70, ("--device-records",))])
def test_device_parse_on_a_cohort_past_one_wavefront(cohort, args, n_smpl, extra):
    d, vcf = cohort
    cmd = [CALL_EXE] + args.format(D=str(d)).split() + [vcf]
    text, count = same_with_and_without(cmd, modes=("u",) if extra else ("v", "u"), extra=extra)
    if extra:                                                   # --device-records -O u: the records as text again
        text = subprocess.run([VIEW_EXE, "-"], input=text, check=True, stdout=subprocess.PIPE).stdout
    recs = [ln.split(b"\t") for ln in text.splitlines() if not ln.startswith(b"#")]
    assert count >= 200 and 0 < len(recs) <= count and all(len(r) == 9 + n_smpl for r in recs)
    assert len(recs) < count or "-v" not in args
    if "--ploidy" in args:
        assert all(b"/" not in c.split(b":")[0] for r in recs for c in r[9:])
    if "GQ" in args:
        assert any(r[8].endswith(b":GP:GQ") for r in recs)
    if "reversed" in args:
        hdr = [ln for ln in text.splitlines() if ln.startswith(b"#CHROM")][0].split(b"\t")
        assert hdr[9] == b"c69" and hdr[-1] == b"c00"


def test_a_line_with_a_column_missing_is_malformed(golden_dir, tmp_path):
    build_host()
    lines = open(os.path.join(golden_dir, "call", "mpileup.vcf")).read().splitlines()
    data = [i for i, ln in enumerate(lines) if not ln.startswith("#")]
    k = data[len(data) // 2]
    lines[k] = lines[k].rsplit("\t", 1)[0]
    bad = str(tmp_path / "bad.vcf")
    open(bad, "w").write("\n".join(lines) + "\n")
    for opt in ([], [OPT]):
        r = subprocess.run([CALL_EXE] + opt + ["-v", bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode != 0 and b"malformed VCF" in r.stderr, (opt, r.stderr)


def test_a_value_that_is_no_integer_is_malformed_with_the_option(golden_dir, tmp_path):
    """Where the option is stricter than the host's atoi: a PL value with a byte that is no digit."""
    build_host()
    lines = open(os.path.join(golden_dir, "call", "mpileup.vcf")).read().splitlines()
    k = [i for i, ln in enumerate(lines) if not ln.startswith("#")][3]
    f = lines[k].split("\t")
    ipl = f[8].split(":").index("PL")
    c = f[-1].split(":")
    c[ipl] = c[ipl] + "x"
    f[-1] = ":".join(c)
    lines[k] = "\t".join(f)
    bad = str(tmp_path / "bad.vcf")
    open(bad, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([CALL_EXE, OPT, "-v", bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"malformed VCF" in r.stderr


def test_without_the_option_timing_prints_what_it_printed(golden_dir):
    build_host()
    vcf = os.path.join(golden_dir, "call", "mpileup.vcf")
    plain = subprocess.run([CALL_EXE, "-v", vcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    timed = subprocess.run([CALL_EXE, "-v", "--timing", vcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert timed.stdout == plain.stdout and plain.stderr == b""
    lines = timed.stderr.decode().splitlines()
    assert len(lines) == 3
    assert re.fullmatch(r"\[bcfgpu_call\] seconds: reading records [\d.]+, building the planes on the host [\d.]+, uploads and device stages [\d.]+, writing records [\d.]+", lines[0])
    assert lines[1] == "[bcfgpu_call] device input: 0 records' planes decoded on the device"
    assert re.fullmatch(r"\[bcfgpu_call\] device records: 0 records' FORMAT blocks encoded on the device", lines[2])
    quiet = subprocess.run([CALL_EXE, OPT, "-v", vcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert quiet.stdout == plain.stdout and quiet.stderr == b""
    with_opt = subprocess.run([CALL_EXE, OPT, "-v", "--timing", vcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE).stderr.decode().splitlines()
    assert len(with_opt) == 4 and with_opt[1:3] == lines[1:3] and with_opt[3] == "[bcfgpu_call] device parse: %d records' planes parsed on the device" % kept_records(vcf)


def test_usage_names_the_option():
    build_host()
    r = subprocess.run([CALL_EXE], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"[--device-parse]" in r.stderr
    for o in (b"[--device-input]", b"[--device-records]", b"[--device-keys]", b"[--device-text]", b"[--timing]", b"[-O v|z|u|b]"):
        assert o in r.stderr
