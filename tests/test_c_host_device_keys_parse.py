"""`bcfgpu_call --device-parse --device-records --device-keys`: text in, BCF out.  With --device-parse and --device-records both in
effect the columns' text stays in HBM after the decode and the integer FORMAT keys the caller passes through (AD, ADF, ADR, DP, SP,
...) are not split, printed again and parsed a second time on the host -- bcfgpu_call_parse_keys_vcf makes their BCF2 key blocks there
from the input records' own columns (the -S sample choice and the Number=R trimming included) and the host splices them between the
device's GT / PL / GQ blocks and the blocks of the keys left to it (Float, String, GP, and a key one of whose values the exact integer
grammar refuses).  The twin of tests/test_c_host_device_keys.py on text input: the output must be the output without any option, byte
for byte, and the reference's goldens: every argument row of the `call -m` goldens on the .vcf itself with -O u and -O b, a 70-sample
cohort with five pass-through keys as text, bgzipped input, stdin and the pipe from bcfgpu_sam, a file with values outside the
grammar, and the runs in which the option does nothing.  --timing's "device keys" line counts the key blocks made on the device
and on the host."""
import os
import re
import subprocess

import pytest

from tests.test_c_host import CALL_EXE, SAM_EXE, VIEW_EXE, build_host, normalised
from tests.test_c_host_device_call_records import CALL_ROWS, as_text, device_count, n_records
from tests.test_c_host_device_keys import COHORT_KEYS, cohort, expected_counts, integer_keys  # noqa: F401  (the 70-sample fixture)

pytestmark = pytest.mark.gpu

ALL = ["--device-parse", "--device-records", "--device-keys"]
AD_INPUTS = ("call-G.vcf", "mpileup.hwe.vcf", "mpileup.NA19213.NA19129.vcf")
KEYS_LINE = rb"\[bcfgpu_call\] device keys: (\d+) pass-through key blocks made on the device, (\d+) on the host\n"


def key_counts(stderr, parse_given=True):
    """(N, M) of the --device-keys line; the lines that were there are still there, in their order, and nothing else."""
    lines = stderr.split(b"\n")
    want = [b"[bcfgpu_call] seconds: reading records ", b"[bcfgpu_call] device input: ", b"[bcfgpu_call] device records: "]
    want += [b"[bcfgpu_call] device parse: "] if parse_given else []
    want += [b"[bcfgpu_call] device keys: "]
    assert len(lines) == len(want) + 1 and lines[-1] == b"" and all(ln.startswith(w) for ln, w in zip(lines, want)), stderr
    m = re.search(KEYS_LINE, stderr)
    assert m, stderr
    return int(m.group(1)), int(m.group(2))


def same_with_and_without(cmd, modes=("u", "b"), opts=ALL, stdin=None):
    """cmd -O u and -O b without any option and with `opts`: the same bytes on stdout.  Returns (the -O u output as text, (N, M),
    the records the device encoded)."""
    text = counts = n_enc = None
    for mode in modes:
        plain = subprocess.run(cmd[:1] + ["-O", mode] + cmd[1:], input=stdin, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        dev = subprocess.run(cmd[:1] + list(opts) + ["--timing", "-O", mode] + cmd[1:], input=stdin, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert plain.stderr == b""
        assert dev.stdout == plain.stdout, mode
        assert counts is None or counts == key_counts(dev.stderr, "--device-parse" in opts)
        counts, n_enc = key_counts(dev.stderr, "--device-parse" in opts), device_count(dev.stderr)
        text = text or as_text(plain.stdout)
    return text, counts, n_enc


@pytest.mark.parametrize("vcff,goldf,args", CALL_ROWS, ids=["%s:%s" % (r[1], r[2].replace("{G}/", "")) for r in CALL_ROWS])
def test_device_keys_on_every_call_golden_as_text(golden_dir, vcff, goldf, args):
    build_host()
    G = os.path.join(golden_dir, "call")
    cmd = [CALL_EXE] + args.format(G=G).split() + [os.path.join(G, vcff)]
    text, counts, n_enc = same_with_and_without(cmd)
    assert normalised(text) == normalised(open(os.path.join(G, goldf)).read()) and n_records(text) > 0
    if args == "-mg0":                                          # -g: none of the three options does anything
        assert counts == (0, 0) and n_enc == 0
    else:
        assert counts == expected_counts(text, integer_keys(open(os.path.join(G, vcff)).read())) and n_enc == n_records(text)
        assert counts[0] > 0 or vcff not in AD_INPUTS                                                       # (FORMAT/AD)


@pytest.fixture(scope="module")
def cohort_text(cohort):  # noqa: F811
    """The 70-sample cohort as `bcfgpu_sam -a AD,ADF,ADR,DP,SP -O v` writes it: the BCF fixture's records as VCF text."""
    d = cohort
    vcf = str(d / "keys.vcf")
    subprocess.check_call([VIEW_EXE, "-O", "v", "-o", vcf, str(d / "keys.bcf")])
    assert open(vcf, "rb").read(2) == b"##"
    return d, vcf


@pytest.mark.parametrize("args,n_smpl", [("-v", 70), ("", 70), ("-v -S {D}/reversed.txt", 70), ("-S {D}/three.txt", 3),
                                         ("-v -G {D}/groups.txt --group-samples-tag AD", 70), ("--ploidy 1", 70), ("-v -a GQ,GP", 70)])
def test_device_keys_on_a_text_cohort_past_one_wavefront(cohort_text, args, n_smpl):
    d, vcf = cohort_text
    cmd = [CALL_EXE] + args.format(D=str(d)).split() + [vcf]
    text, (n_dev, n_host), n_enc = same_with_and_without(cmd, modes=("u",))
    recs = [ln.split("\t") for ln in text.splitlines() if not ln.startswith("#")]
    assert n_enc == len(recs) > 0 and all(len(r) == 9 + n_smpl for r in recs)
    assert len(recs) >= 200 or "-v" in args
    assert all(set(COHORT_KEYS) <= set(r[8].split(":")) for r in recs)
    assert n_dev == len(recs) * len(COHORT_KEYS) > 0                # records written x integer pass-through keys
    if "GP" in args:
        assert n_host == sum("GP" in r[8].split(":") for r in recs) > 0
    else:
        assert n_host == 0
    for r in recs:                                                  # alleles were dropped: the Number=R keys follow them
        keys = r[8].split(":")
        for k in ("AD", "ADF", "ADR"):
            assert len(r[9].split(":")[keys.index(k)].split(",")) == 1 + (0 if r[4] == "." else len(r[4].split(","))), r[:10]


def test_device_keys_on_bgzipped_input_stdin_and_the_pipe_from_bcfgpu_sam(golden_dir, tmp_path):
    build_host()
    G = os.path.join(golden_dir, "call")
    vcf = os.path.join(G, "mpileup.hwe.vcf")
    gz = str(tmp_path / "in.vcf.gz")
    subprocess.check_call([VIEW_EXE, "-O", "z", "-o", gz, vcf])
    assert open(gz, "rb").read(2) == b"\x1f\x8b"
    text, counts, n_enc = same_with_and_without([CALL_EXE, "-v", vcf], modes=("u",))
    want = expected_counts(text, integer_keys(open(vcf).read()))
    assert counts == want and want[0] > 0 and n_enc == n_records(text)
    assert same_with_and_without([CALL_EXE, "-v", gz], modes=("u",)) == (text, counts, n_enc)
    for data in (open(vcf, "rb").read(), open(gz, "rb").read()):
        assert same_with_and_without([CALL_EXE, "-v", "-"], modes=("u",), stdin=data) == (text, counts, n_enc)
    # `bcfgpu_sam -a AD,DP -O v ... | bcfgpu_call --device-parse --device-records --device-keys -v -O u -` against the same through a file, no option
    M = os.path.join(golden_dir, "mpileup")
    sam_cmd = [SAM_EXE, "-a", "AD,DP", "-O", "v", "-f", os.path.join(M, "mpileup.ref.fa"), "-r", "17:100-600"] + [os.path.join(M, "mpileup.%d.sam" % i) for i in (1, 2, 3)]
    m_vcf = str(tmp_path / "m.vcf")
    with open(m_vcf, "wb") as f:
        subprocess.run(sam_cmd, check=True, stdout=f)
    via_file = subprocess.run([CALL_EXE, "-v", "-O", "u", m_vcf], check=True, stdout=subprocess.PIPE).stdout
    p1 = subprocess.Popen(sam_cmd, stdout=subprocess.PIPE)
    via_pipe = subprocess.run([CALL_EXE] + ALL + ["--timing", "-v", "-O", "u", "-"], stdin=p1.stdout, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    p1.stdout.close()
    assert p1.wait() == 0
    assert via_pipe.stdout == via_file
    n = n_records(as_text(via_file))
    assert key_counts(via_pipe.stderr) == (2 * n, 0) and n >= 1


def test_values_outside_the_grammar_go_back_to_the_host(cohort_text, tmp_path):
    """`12x`, an empty value and `99999999999` planted in the AD and DP tokens of three records that are written: the bytes are those
    of the run without options, and exactly those keys are counted on the host."""
    d, vcf = cohort_text
    plain = as_text(subprocess.run([CALL_EXE, "-O", "u", vcf], check=True, stdout=subprocess.PIPE).stdout)
    n = n_records(plain)
    lines = open(vcf).read().splitlines()
    data = [i for i, ln in enumerate(lines) if not ln.startswith("#")]
    assert len(data) == n                                           # (without -v every record is written)
    plant = [(data[3], "AD", 5, 0, "12x"), (data[n // 2], "DP", 40, 0, ""), (data[n // 2], "AD", 68, 1, "99999999999"), (data[n - 2], "DP", 0, 0, "99999999999")]
    for i, key, s, j, bad in plant:
        f = lines[i].split("\t")
        toks = f[9 + s].split(":")
        k = f[8].split(":").index(key)
        v = toks[k].split(",")
        v[j] = bad
        toks[k] = ",".join(v)
        f[9 + s] = ":".join(toks)
        lines[i] = "\t".join(f)
    bad_vcf = str(tmp_path / "planted.vcf")
    open(bad_vcf, "w").write("\n".join(lines) + "\n")
    text, (n_dev, n_host), n_enc = same_with_and_without([CALL_EXE, bad_vcf], modes=("u",))
    assert n_enc == n_records(text) == n
    assert (n_dev, n_host) == (n * len(COHORT_KEYS) - len(plant), len(plant))
    for args in ("-S {D}/three.txt", "-v -S {D}/reversed.txt"):     # the three called samples have none of the planted columns: nothing is flagged
        text, (n_dev, n_host), n_enc = same_with_and_without([CALL_EXE] + args.format(D=str(d)).split() + [bad_vcf], modes=("u",))
        flagged = 0 if "three" in args else sum(1 for i, *_ in plant if any(ln.split("\t")[1] == lines[i].split("\t")[1] for ln in text.splitlines() if not ln.startswith("#")))
        assert (n_dev, n_host) == (n_records(text) * len(COHORT_KEYS) - flagged, flagged)


NOTHING = [("without-device-parse", "-v {vcf}", "u", ALL[1:], False), ("device-input-on-text-input", "-v {vcf}", "u", ["--device-input"] + ALL[1:], False),
           ("without-device-records", "-v {vcf}", "u", [ALL[0], ALL[2]], True), ("text-output", "-v {vcf}", "v", ALL, True),
           ("gvcf", "-g 0 {vcf}", "u", ALL, True), ("constrained-alleles", "-m -A -C alleles -T {G}/mpileup.tab {vcf}", "u", ALL, True)]


@pytest.mark.parametrize("tail,mode,opts,parse_given", [r[1:] for r in NOTHING], ids=[r[0] for r in NOTHING])
def test_the_option_does_nothing_where_it_should(golden_dir, tail, mode, opts, parse_given):
    """Without --device-parse on text input, without --device-records, -O v, -g, -C alleles: the same bytes and no device key block."""
    build_host()
    G = os.path.join(golden_dir, "call")
    vcf = os.path.join(G, "mpileup.vcf" if "alleles" in tail else "mpileup.hwe.vcf")
    tail = tail.format(G=G, vcf=vcf).split()
    plain = subprocess.run([CALL_EXE, "-O", mode] + tail, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    dev = subprocess.run([CALL_EXE] + opts + ["--timing", "-O", mode] + tail, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert plain.stderr == b"" and dev.stdout == plain.stdout and len(plain.stdout) > 0
    assert key_counts(dev.stderr, parse_given)[0] == 0


def test_stderr_without_the_option_and_without_timing(golden_dir):
    """Without --device-keys --timing prints the four lines it printed before, word for word; without --timing nothing is printed."""
    build_host()
    vcf = os.path.join(golden_dir, "call", "mpileup.hwe.vcf")
    base = [CALL_EXE, "-v", "-O", "u"]
    quiet = subprocess.run(base + ALL + [vcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    off = subprocess.run(base + ALL[:2] + ["--timing", vcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    on = subprocess.run(base + ALL + ["--timing", vcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert quiet.stderr == b"" and quiet.stdout == off.stdout == on.stdout
    lines = off.stderr.split(b"\n")
    assert len(lines) == 5 and lines[4] == b"" and b"device keys" not in off.stderr
    assert lines[0].startswith(b"[bcfgpu_call] seconds: reading records ") and lines[1] == b"[bcfgpu_call] device input: 0 records' planes decoded on the device"
    assert lines[2].startswith(b"[bcfgpu_call] device records: ") and lines[3].startswith(b"[bcfgpu_call] device parse: ")
    assert re.fullmatch(rb"\[bcfgpu_call\] seconds: reading records [\d.]+, building the planes on the host [\d.]+, uploads and device stages [\d.]+, writing records [\d.]+", lines[0])
    assert [re.sub(rb"[\d.]+", b"#", x) for x in on.stderr.split(b"\n")[:4]] == [re.sub(rb"[\d.]+", b"#", x) for x in lines[:4]]
    assert key_counts(on.stderr)[0] > 0
