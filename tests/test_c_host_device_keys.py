"""`bcfgpu_call --device-keys`: with --device-input and --device-records both in effect, the integer FORMAT keys the caller passes
through (AD, ADF, ADR, DP, SP, ...) are not printed, split, re-ordered and parsed back on the host -- bcfgpu_call_remap_bcf makes
their BCF2 key blocks in HBM from the input records' bytes (the -S sample choice and the Number=R trimming included) and the host
splices them between the device's GT / PL / GQ blocks and the blocks of the keys left to it (Float, String, GP).  The output must be
the output without any option, byte for byte, and the reference's goldens: every argument row of the `call -m` goldens on BCF input
with -O u and -O b, a 70-sample cohort with five pass-through keys, the runs in which the option does nothing, and the pipe from
bcfgpu_sam.  --timing's extra line counts the key blocks made on the device and on the host."""
import os
import re
import subprocess

import pytest

from tests.test_c_host import CALL_EXE, SAM_EXE, build_host, normalised
from tests.test_c_host_device_call_records import CALL_ROWS, as_text, device_count, n_records, to_bcf
from tests.test_c_host_device_records import _cohort_sam

pytestmark = pytest.mark.gpu

ALL = ["--device-input", "--device-records", "--device-keys"]
COHORT_KEYS = ["AD", "ADF", "ADR", "DP", "SP"]


def key_counts(stderr):
    """(N, M) of the --device-keys line; the three lines that were there are still there, and nothing else."""
    assert b"reading records" in stderr and b"device input: " in stderr and b"device records: " in stderr
    m = re.search(rb"\[bcfgpu_call\] device keys: (\d+) pass-through key blocks made on the device, (\d+) on the host\n", stderr)
    assert m and stderr.count(b"\n") == 4, stderr
    return int(m.group(1)), int(m.group(2))


def same_with_and_without(cmd, modes=("u", "b"), opts=ALL):
    """cmd -O u and -O b without any option and with `opts`: the same bytes on stdout.  Returns (the -O u output as text, (N, M),
    the records the device encoded)."""
    text = counts = n_enc = None
    for mode in modes:
        plain = subprocess.run(cmd[:1] + ["-O", mode] + cmd[1:], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        dev = subprocess.run(cmd[:1] + list(opts) + ["--timing", "-O", mode] + cmd[1:], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert plain.stderr == b""
        assert dev.stdout == plain.stdout, mode
        assert counts is None or counts == key_counts(dev.stderr)
        counts, n_enc = key_counts(dev.stderr), device_count(dev.stderr)
        text = text or as_text(plain.stdout)
    return text, counts, n_enc


def integer_keys(text):
    """The FORMAT keys, other than PL and GT, that the header of a VCF text declares Type=Integer."""
    return {m.group(1) for m in re.finditer(r"^##FORMAT=<ID=([^,]+),Number=[^,]+,Type=Integer", text, flags=re.M)} - {"PL", "GT"}


def expected_counts(text, input_keys):
    """(device, host) key blocks of the records of `text`: the input's integer keys on the device; the rest but GT, PL and GQ on the host."""
    n = m = 0
    for ln in text.splitlines():
        if ln.startswith("#") or not ln:
            continue
        for k in ln.split("\t")[8].split(":"):
            n += k in input_keys
            m += k not in input_keys and k not in ("GT", "PL", "GQ")
    return n, m


@pytest.mark.parametrize("vcff,goldf,args", CALL_ROWS, ids=["%s:%s" % (r[1], r[2].replace("{G}/", "")) for r in CALL_ROWS])
def test_device_keys_on_every_call_golden(golden_dir, tmp_path, vcff, goldf, args):
    build_host()
    G = os.path.join(golden_dir, "call")
    bcf = to_bcf(os.path.join(G, vcff), str(tmp_path / "in.bcf"))
    cmd = [CALL_EXE] + args.format(G=G).split() + [bcf]
    text, counts, n_enc = same_with_and_without(cmd)
    assert normalised(text) == normalised(open(os.path.join(G, goldf)).read()) and n_records(text) > 0
    if args == "-mg0":                                          # -g: none of the three options does anything
        assert counts == (0, 0) and n_enc == 0
    else:
        assert counts == expected_counts(text, integer_keys(open(os.path.join(G, vcff)).read())) and n_enc == n_records(text)
        assert counts[0] > 0 or vcff not in ("call-G.vcf", "mpileup.hwe.vcf", "mpileup.NA19213.NA19129.vcf")       # (FORMAT/AD)


@pytest.fixture(scope="module")
def cohort(golden_dir, tmp_path_factory):
    """The 70 single-sample files of tests/test_c_host_device_call_records.py over 200 columns through `bcfgpu_sam -O u` with
    -a AD,ADF,ADR,DP,SP: five integer pass-through keys, three of them Number=R."""
    build_host()
    d = tmp_path_factory.mktemp("cohort")
    G = os.path.join(golden_dir, "mpileup")
    ref = "".join(ln.strip() for ln in open(os.path.join(G, "mpileup.ref.fa")) if not ln.startswith(">"))
    files = []
    for s in range(70):
        files.append(str(d / ("c%02d.sam" % s)))
        _cohort_sam(files[-1], ref, "c%02d" % s, 1000 + s, 1000, 1200)
    subprocess.check_call([SAM_EXE, "-a", ",".join(COHORT_KEYS), "-O", "u", "-o", str(d / "keys.bcf"), "-f", os.path.join(G, "mpileup.ref.fa"), "-r", "17:1001-1200"] + files)
    names = ["c%02d" % s for s in range(70)]
    (d / "reversed.txt").write_text("".join(n + "\n" for n in names[::-1]))
    (d / "three.txt").write_text("c41\nc03\nc69\n")
    (d / "groups.txt").write_text("".join("%s\t%s\n" % (n, "even" if i % 2 == 0 else "odd") for i, n in enumerate(names)))
    return d


@pytest.mark.parametrize("args,n_smpl", [("-v", 70), ("", 70), ("-v -S {D}/reversed.txt", 70), ("-S {D}/three.txt", 3),
                                         ("-v -G {D}/groups.txt --group-samples-tag AD", 70), ("--ploidy 1", 70), ("-v -a GQ,GP", 70)])
def test_device_keys_on_a_cohort_past_one_wavefront(cohort, args, n_smpl):
    d = cohort
    cmd = [CALL_EXE] + args.format(D=str(d)).split() + [str(d / "keys.bcf")]
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


NOTHING = [("text-input", "-v {vcf}", "u", ALL), ("text-output", "-v {bcf}", "v", ALL), ("gvcf", "-g 0 {bcf}", "u", ALL),
           ("constrained-alleles", "-m -A -C alleles -T {G}/mpileup.tab {bcf}", "u", ALL), ("alone", "-v {bcf}", "u", ALL[2:]),
           ("without-device-input", "-v {bcf}", "u", ALL[1:]), ("without-device-records", "-v {bcf}", "u", [ALL[0], ALL[2]])]


@pytest.mark.parametrize("tail,mode,opts", [r[1:] for r in NOTHING], ids=[r[0] for r in NOTHING])
def test_the_option_does_nothing_where_it_should(golden_dir, tmp_path, tail, mode, opts):
    """Text input, -O v, -g, -C alleles, and the option alone or with one of the other two: the same bytes and no device key block."""
    build_host()
    G = os.path.join(golden_dir, "call")
    vcf = os.path.join(G, "mpileup.vcf" if "alleles" in tail else "mpileup.hwe.vcf")
    tail = tail.format(G=G, vcf=vcf, bcf=to_bcf(vcf, str(tmp_path / "in.bcf")) if "{bcf}" in tail else None).split()
    plain = subprocess.run([CALL_EXE, "-O", mode] + tail, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    dev = subprocess.run([CALL_EXE] + opts + ["--timing", "-O", mode] + tail, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert plain.stderr == b"" and dev.stdout == plain.stdout and len(plain.stdout) > 0
    assert key_counts(dev.stderr)[0] == 0


def test_stderr_without_the_option_and_without_timing(golden_dir, tmp_path):
    """Without --device-keys --timing prints the three lines it printed before; without --timing nothing is printed."""
    build_host()
    G = os.path.join(golden_dir, "call")
    bcf = to_bcf(os.path.join(G, "mpileup.hwe.vcf"), str(tmp_path / "in.bcf"))
    base = [CALL_EXE, "-v", "-O", "u"]
    quiet = subprocess.run(base + ALL + [bcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    off = subprocess.run(base + ALL[:2] + ["--timing", bcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    on = subprocess.run(base + ALL + ["--timing", bcf], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert quiet.stderr == b"" and quiet.stdout == off.stdout == on.stdout
    lines = off.stderr.split(b"\n")
    assert len(lines) == 4 and lines[3] == b"" and b"device keys" not in off.stderr
    assert lines[0].startswith(b"[bcfgpu_call] seconds: reading records ") and lines[1].startswith(b"[bcfgpu_call] device input: ")
    assert lines[2].startswith(b"[bcfgpu_call] device records: ")
    assert [re.sub(rb"[\d.]+", b"#", x) for x in on.stderr.split(b"\n")[:3]] == [re.sub(rb"[\d.]+", b"#", x) for x in lines[:3]]
    assert key_counts(on.stderr)[0] > 0


def test_device_keys_from_the_pipe(golden_dir, tmp_path):
    """`bcfgpu_sam -a AD,DP -O u ... | bcfgpu_call --device-input --device-records --device-keys -v -O u -` against the same through a
    file with no option."""
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    sam_cmd = [SAM_EXE, "-a", "AD,DP", "-O", "u", "-f", os.path.join(G, "mpileup.ref.fa"), "-r", "17:100-600"] + [os.path.join(G, "mpileup.%d.sam" % i) for i in (1, 2, 3)]
    bcf = str(tmp_path / "m.bcf")
    with open(bcf, "wb") as f:
        subprocess.run(sam_cmd, check=True, stdout=f)
    via_file = subprocess.run([CALL_EXE, "-v", "-O", "u", bcf], check=True, stdout=subprocess.PIPE).stdout
    p1 = subprocess.Popen(sam_cmd, stdout=subprocess.PIPE)
    via_pipe = subprocess.run([CALL_EXE] + ALL + ["--timing", "-v", "-O", "u", "-"], stdin=p1.stdout, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    p1.stdout.close()
    assert p1.wait() == 0
    assert via_pipe.stdout == via_file
    n = n_records(as_text(via_file))
    assert key_counts(via_pipe.stderr) == (2 * n, 0) and n >= 1
