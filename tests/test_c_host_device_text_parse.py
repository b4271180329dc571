"""`bcfgpu_call --device-parse --device-text`: text in, text out.  With -O v|z and --device-parse in effect the columns' text stays in
HBM after the decode and the sample columns of the written records are rewritten there (bcfgpu_call_rewrite_vcf: GT, the input
column's tokens in their order with the trimmed PL in PL's place, the Number=R tokens following the alleles, GQ); the host prints the
head alone.  A Float or String key keeps no record from the device; a record with GP stays on the host.  The output must be the
output without any option, byte for byte, and the reference's goldens: every argument row of the `call -m` goldens on the .vcf itself
with -O v and -O z, a 70-sample cohort with five pass-through keys as text, a record with a Float and a String key, input that is
plain, bgzipped and on a pipe from bcfgpu_sam, the runs in which the option does nothing, and a malformed record.  --timing's
"device text" line counts the records rewritten on the device and left to the host."""
import os
import subprocess

import pytest

from tests.test_c_host import CALL_EXE, SAM_EXE, VIEW_EXE, build_host, normalised
from tests.test_c_host_device_call_records import CALL_ROWS, n_records, to_bcf
from tests.test_c_host_device_keys import COHORT_KEYS, cohort  # noqa: F401  (the 70-sample fixture)
from tests.test_c_host_device_text_call import FLOAT_VCF, records, same_with_and_without, text_counts

pytestmark = pytest.mark.gpu

OPTS = ["--device-parse", "--device-text"]
LINES = 5                                                           # of --timing: the three that always come, device parse, device text


@pytest.mark.parametrize("vcff,goldf,args", CALL_ROWS, ids=["%s:%s" % (r[1], r[2].replace("{G}/", "")) for r in CALL_ROWS])
def test_device_text_on_every_call_golden_as_text(golden_dir, vcff, goldf, args):
    build_host()
    G = os.path.join(golden_dir, "call")
    cmd = [CALL_EXE] + args.format(G=G).split() + [os.path.join(G, vcff)]
    text, (n_dev, n_host) = same_with_and_without(cmd, opts=OPTS, lines=LINES)
    assert normalised(text) == normalised(open(os.path.join(G, goldf)).read()) and n_records(text) > 0
    if args == "-mg0":                                          # -g: neither option does anything
        assert n_dev == 0
    else:
        recs = records(text)
        assert n_dev + n_host == len(recs)
        assert n_host == sum("GP" in r[8].split(":") for r in recs)
        assert n_dev > 0 or "GP" in args


@pytest.fixture(scope="module")
def cohort_text(cohort):  # noqa: F811
    d = cohort
    vcf = str(d / "keys.vcf")
    subprocess.check_call([VIEW_EXE, "-O", "v", "-o", vcf, str(d / "keys.bcf")])
    assert open(vcf, "rb").read(2) == b"##"
    return d, vcf


@pytest.mark.parametrize("args,n_smpl", [("-v", 70), ("", 70), ("-v -S {D}/reversed.txt", 70), ("-S {D}/three.txt", 3),
                                         ("-v -G {D}/groups.txt --group-samples-tag AD", 70), ("--ploidy 1", 70), ("-v -a GQ,GP", 70), ("-a GQ,GP", 70)])
def test_device_text_on_a_text_cohort_past_one_wavefront(cohort_text, args, n_smpl):
    d, vcf = cohort_text
    cmd = [CALL_EXE] + args.format(D=str(d)).split() + [vcf]
    text, (n_dev, n_host) = same_with_and_without(cmd, modes=("v",), opts=OPTS, lines=LINES)
    recs = records(text)
    assert n_dev + n_host == len(recs) > 0 and all(len(r) == 9 + n_smpl for r in recs)
    assert len(recs) >= 200 or "-v" in args
    assert all(set(COHORT_KEYS) <= set(r[8].split(":")) for r in recs)
    if "GP" in args:
        assert n_host == sum("GP" in r[8].split(":") for r in recs) > 0
        assert n_dev == (0 if "-v" in args else sum("GP" not in r[8].split(":") for r in recs)) and ("-v" in args or n_dev > 0)
    else:
        assert n_host == 0
    for r in recs:                                                  # alleles were dropped: the Number=R keys follow them
        keys = r[8].split(":")
        for k in ("AD", "ADF", "ADR"):
            assert len(r[9].split(":")[keys.index(k)].split(",")) == 1 + (0 if r[4] == "." else len(r[4].split(","))), r[:10]


STRING_VCF = FLOAT_VCF.replace('##FORMAT=<ID=XF,Number=1,Type=Float,Description="x">\n',
                               '##FORMAT=<ID=XF,Number=1,Type=Float,Description="x">\n##FORMAT=<ID=XS,Number=1,Type=String,Description="x">\n') \
                      .replace("\tPL:AD\t0,30,200,30,200,200:10,0,0\t200,30,0,200,30,200:0,10,0", "\tPL:XS:AD\t0,30,200,30,200,200:left,x:10,0,0\t200,30,0,200,30,200:.:0,10,0")


def test_records_with_a_float_and_a_string_key_are_the_devices(tmp_path):
    """What the BCF route leaves to the host for the key's type is a token like any other here."""
    build_host()
    assert "XS" in STRING_VCF and "left,x" in STRING_VCF
    vcf = str(tmp_path / "float.vcf")
    open(vcf, "w").write(STRING_VCF)
    text, counts = same_with_and_without([CALL_EXE, vcf], opts=OPTS, lines=LINES)
    recs = records(text)
    assert len(recs) == 2 and recs[0][8] == "GT:PL:AD:XF" and recs[1][8] == "GT:PL:XS:AD" and counts == (2, 0)
    assert recs[0][9].endswith(":0.5") and recs[0][10].endswith(":1.25") and (recs[0][4], recs[1][4]) == ("C", "T")
    assert recs[1][9].split(":")[2:] == ["left,x", "10,0"] and recs[1][10].split(":")[2:] == [".", "0,10"]


def test_device_text_on_bgzipped_input_stdin_and_the_pipe_from_bcfgpu_sam(golden_dir, tmp_path):
    build_host()
    G = os.path.join(golden_dir, "call")
    vcf = os.path.join(G, "mpileup.vcf")
    gz = str(tmp_path / "in.vcf.gz")
    subprocess.check_call([VIEW_EXE, "-O", "z", "-o", gz, vcf])
    assert open(gz, "rb").read(2) == b"\x1f\x8b"
    want = normalised(open(os.path.join(G, "mpileup.1.out")).read())
    text, (n_dev, n_host) = same_with_and_without([CALL_EXE, "-v", gz], opts=OPTS, lines=LINES)
    assert normalised(text) == want and (n_dev, n_host) == (n_records(text), 0)
    for data in (open(vcf, "rb").read(), open(gz, "rb").read()):
        plain = subprocess.run([CALL_EXE, "-v", "-O", "v", "-"], input=data, check=True, stdout=subprocess.PIPE).stdout
        dev = subprocess.run([CALL_EXE] + OPTS + ["--timing", "-v", "-O", "v", "-"], input=data, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert dev.stdout == plain and normalised(plain.decode()) == want and text_counts(dev.stderr, LINES) == (n_records(text), 0)
    # `bcfgpu_sam -a AD,DP -O v ... | bcfgpu_call --device-parse --device-text -v -O v -` against the same through a file, no option
    M = os.path.join(golden_dir, "mpileup")
    sam_cmd = [SAM_EXE, "-a", "AD,DP", "-O", "v", "-f", os.path.join(M, "mpileup.ref.fa"), "-r", "17:100-600"] + [os.path.join(M, "mpileup.%d.sam" % i) for i in (1, 2, 3)]
    m_vcf = str(tmp_path / "m.vcf")
    with open(m_vcf, "wb") as f:
        subprocess.run(sam_cmd, check=True, stdout=f)
    via_file = subprocess.run([CALL_EXE, "-v", "-O", "v", m_vcf], check=True, stdout=subprocess.PIPE).stdout
    p1 = subprocess.Popen(sam_cmd, stdout=subprocess.PIPE)
    via_pipe = subprocess.run([CALL_EXE] + OPTS + ["--timing", "-v", "-O", "v", "-"], stdin=p1.stdout, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    p1.stdout.close()
    assert p1.wait() == 0
    assert via_pipe.stdout == via_file
    n = n_records(via_file.decode())
    assert text_counts(via_pipe.stderr, LINES) == (n, 0) and n >= 1


NOTHING = [("gvcf", "-g 0 {vcf}", "v", OPTS, 5), ("constrained-alleles", "-m -A -C alleles -T {G}/mpileup.tab {vcf}", "v", OPTS, 5),
           ("bcf-output", "-v {vcf}", "u", OPTS, 5), ("without-device-parse", "-v {vcf}", "v", OPTS[1:], 4),
           ("device-input-on-text-input", "-v {vcf}", "v", ["--device-input", "--device-text"], 4)]


@pytest.mark.parametrize("tail,mode,opts,lines", [r[1:] for r in NOTHING], ids=[r[0] for r in NOTHING])
def test_the_option_does_nothing_where_it_should(golden_dir, tail, mode, opts, lines):
    """-g, -C alleles, -O u, and --device-text without --device-parse on text input: the same bytes, no record rewritten on the device."""
    build_host()
    G = os.path.join(golden_dir, "call")
    vcf = os.path.join(G, "mpileup.vcf" if "alleles" in tail else "mpileup.hwe.vcf")
    tail = tail.format(G=G, vcf=vcf).split()
    plain = subprocess.run([CALL_EXE, "-O", mode] + tail, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    dev = subprocess.run([CALL_EXE] + opts + ["--timing", "-O", mode] + tail, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert plain.stderr == b"" and dev.stdout == plain.stdout and len(plain.stdout) > 0
    assert text_counts(dev.stderr, lines)[0] == 0


def test_device_parse_on_bcf_input_leaves_device_text_to_device_input(golden_dir, tmp_path):
    """On BCF input --device-parse does nothing: --device-text beside it alone does nothing either, and with --device-input it is
    the BCF route's."""
    build_host()
    G = os.path.join(golden_dir, "call")
    bcf = to_bcf(os.path.join(G, "mpileup.hwe.vcf"), str(tmp_path / "in.bcf"))
    text, (n_dev, _) = same_with_and_without([CALL_EXE, "-v", bcf], opts=OPTS, lines=LINES)
    assert n_dev == 0 and n_records(text) > 0
    text, (n_dev, n_host) = same_with_and_without([CALL_EXE, "-v", bcf], opts=OPTS + ["--device-input"], lines=LINES)
    assert (n_dev, n_host) == (n_records(text), 0)


def test_a_line_with_a_column_missing_is_still_malformed(golden_dir, tmp_path):
    build_host()
    lines = open(os.path.join(golden_dir, "call", "mpileup.vcf")).read().splitlines()
    data = [i for i, ln in enumerate(lines) if not ln.startswith("#")]
    k = data[len(data) // 2]
    lines[k] = lines[k].rsplit("\t", 1)[0]
    bad = str(tmp_path / "bad.vcf")
    open(bad, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([CALL_EXE] + OPTS + ["-v", "-O", "v", bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"malformed VCF" in r.stderr and not [ln for ln in r.stdout.splitlines() if not ln.startswith(b"#")]


def test_usage_and_stderr_without_timing(golden_dir):
    build_host()
    r = subprocess.run([CALL_EXE], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"--device-text acts with -O v|z where --device-input (BCF in) or --device-parse (VCF text in) is in effect" in r.stderr
    vcf = os.path.join(golden_dir, "call", "mpileup.hwe.vcf")
    quiet = subprocess.run([CALL_EXE] + OPTS + ["-v", vcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert quiet.stderr == b"" and n_records(quiet.stdout.decode()) > 0
