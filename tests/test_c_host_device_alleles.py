"""`bcfgpu_call --device-alleles`: with -C alleles -T targets the input options take effect -- the host pairs a record with its target and
rewrites the first nine columns, the samples' bytes (--device-input, BCF in) or text (--device-parse, text in) go to the device as they
are, the decoders make planes of the input records' shape and bcfgpu_call_constrain gathers them into the planes mcall() reads.  The
output must be the output without any option, byte for byte, and the reference's nine `-C alleles` goldens, whole files; with
--device-records, --device-keys and --device-text on top the same bytes again, a changed record's Number=R keys (or its columns) on the
host and the rest on the device; a 70-sample cohort with a targets file made from its own records, with -i, -S and -G; and the runs in
which the option does nothing.  --timing's extra line counts the records constrained on the device and those taken as they were."""
import os
import re
import subprocess

import pytest

from tests.helpers import cals, vcf as V
from tests.test_c_host import CALL_EXE, SAM_EXE, VIEW_EXE, build_host, normalised, whole_file_checks
from tests.test_c_host_device_call_records import as_text, n_records
from tests.test_c_host_device_input import CALS_ROWS, device_count, to_bcf
from tests.test_c_host_device_keys import integer_keys
from tests.test_c_host_device_parse import parse_count
from tests.test_c_host_device_records import _cohort_sam

pytestmark = pytest.mark.gpu

OPT = "--device-alleles"
IN_OPT = {"text": "--device-parse", "bcf": "--device-input"}
ALS_LINE = rb"\[bcfgpu_call\] device alleles: (\d+) records' planes constrained on the device, (\d+) taken as they were\n"
KEYS_LINE = rb"\[bcfgpu_call\] device keys: (\d+) pass-through key blocks made on the device, (\d+) on the host\n"
TEXT_LINE = rb"\[bcfgpu_call\] device text: (\d+) records' sample columns formatted on the device, (\d+) on the host\n"
R_KEYS = ("AD", "ADF", "ADR")


def counts(line, stderr):
    m = re.findall(line, stderr)
    assert len(m) == 1, stderr
    return int(m[0][0]), int(m[0][1])


def decoded(kind, stderr):
    """the records whose planes the input option's line reports"""
    return parse_count(stderr) if kind == "text" else device_count(stderr)


def run(cmd, opts=(), mode="v"):
    return subprocess.run(cmd[:1] + list(opts) + (["--timing"] if opts else []) + ["-O", mode] + cmd[1:], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def cals_cmd(G, vcff, tab, ins, path):
    return [CALL_EXE, "-m", "-A", "-C", "alleles", "-T", os.path.join(G, tab)] + (["-i"] if ins else []) + [path]


def the_input(G, vcff, kind, tmp_path):
    return os.path.join(G, vcff) if kind == "text" else to_bcf(os.path.join(G, vcff), str(tmp_path / "in.bcf"))


def pairing(G, vcff, tab, ins):
    """What the record loop does with the input, restated by tests/helpers/cals.py: [(the record that is called, changed)] in order."""
    vcf = V.Vcf(os.path.join(G, vcff))
    mine = {id(r) for r in vcf.recs}
    ev = cals.constrain(vcf, cals.parse_tab(os.path.join(G, tab)), ins)
    return [(e, id(e) not in mine) for e in ev if not isinstance(e, cals.Missed)]


@pytest.mark.parametrize("kind", ["text", "bcf"])
@pytest.mark.parametrize("vcff,goldf,tab,ins", CALS_ROWS)
def test_device_alleles_on_every_constrained_golden(golden_dir, tmp_path, vcff, goldf, tab, ins, kind):
    build_host()
    G = os.path.join(golden_dir, "call")
    cmd = cals_cmd(G, vcff, tab, ins, the_input(G, vcff, kind, tmp_path))
    opts = [IN_OPT[kind], OPT]
    whole_file_checks(cmd[:1] + opts + cmd[1:], os.path.join(G, goldf))
    paired = pairing(G, vcff, tab, ins)
    for mode in ("v", "u"):
        plain, dev = run(cmd, mode=mode), run(cmd, opts, mode)
        assert plain.stderr == b"" and dev.stdout == plain.stdout, mode
        n, m = counts(ALS_LINE, dev.stderr)
        assert n + m == len(paired) == decoded(kind, dev.stderr) and n == sum(c for _, c in paired) > 0


def written_with_their_records(text, paired):
    """[(the output line's columns, the input record's FORMAT keys, changed)] of the records of `text` that are no -i lines; every paired
    record of these inputs is written (-A, no -v), in order."""
    recs = [ln.split("\t") for ln in text.splitlines() if ln and not ln.startswith("#")]
    recs = [r for r in recs if r[8] != "GT"]
    assert len(recs) == len(paired)
    for r, (e, _) in zip(recs, paired):
        assert (r[0], int(r[1])) == (e.chrom, e.pos)
    return [(r, e.fmt_keys, c) for r, (e, c) in zip(recs, paired)]


@pytest.mark.parametrize("kind", ["text", "bcf"])
@pytest.mark.parametrize("vcff,goldf,tab,ins", CALS_ROWS)
def test_device_alleles_with_the_output_options(golden_dir, tmp_path, vcff, goldf, tab, ins, kind):
    """--device-records and --device-keys (-O u), --device-text (-O v): the same bytes; a changed record's Number=R keys other than PL
    are the host's blocks, and such a record's columns the host's text; everything else is the device's."""
    build_host()
    G = os.path.join(golden_dir, "call")
    cmd = cals_cmd(G, vcff, tab, ins, the_input(G, vcff, kind, tmp_path))
    ints = integer_keys(open(os.path.join(G, vcff)).read())
    paired = pairing(G, vcff, tab, ins)
    plain_u, plain_v = run(cmd, mode="u"), run(cmd, mode="v")
    assert normalised(plain_v.stdout.decode()) == normalised(open(os.path.join(G, goldf)).read())
    rows = written_with_their_records(plain_v.stdout.decode(), paired)
    r_keys = cals._numberR_formats(V.Vcf(os.path.join(G, vcff)).header) - {"PL"}
    assert set(R_KEYS) & r_keys or vcff not in ("mpileup.2.vcf", "mpileup.cals.1.vcf")
    moved = [sum(k in r_keys for k in keys) if changed else 0 for _, keys, changed in rows]     # the keys that follow amap first

    dev = run(cmd, [IN_OPT[kind], OPT, "--device-records"], "u")
    assert dev.stdout == plain_u.stdout and counts(ALS_LINE, dev.stderr)[0] > 0
    assert int(re.search(rb"device records: (\d+) records' FORMAT blocks", dev.stderr).group(1)) == len(rows)
    dev = run(cmd, [IN_OPT[kind], OPT, "--device-records", "--device-keys"], "u")
    assert dev.stdout == plain_u.stdout
    moved_int = sum(sum(k in r_keys and k in ints for k in keys) for _, keys, changed in rows if changed)
    n_dev = sum(sum(k in ints for k in r[8].split(":")) for r, _, _ in rows) - moved_int
    n_host = sum(sum(k not in ints and k not in ("GT", "PL", "GQ") for k in r[8].split(":")) for r, _, _ in rows) + moved_int
    assert counts(KEYS_LINE, dev.stderr) == (n_dev, n_host)
    dev = run(cmd, [IN_OPT[kind], OPT, "--device-text"], "v")
    assert dev.stdout == plain_v.stdout
    n_thost = sum(x > 0 for x in moved)
    assert counts(TEXT_LINE, dev.stderr) == (len(rows) - n_thost, n_thost)
    if vcff in ("mpileup.2.vcf", "mpileup.cals.1.vcf"):            # a changed record with AD / ADF / ADR: those on the host, its DP on the device
        assert n_thost > 0 and moved_int > 0 and n_dev > 0
    if vcff == "mpileup.2.vcf":                                     # ... and records that keep their columns on the device
        assert len(rows) > n_thost


@pytest.fixture(scope="module")
def cohort(golden_dir, tmp_path_factory):
    """70 single-sample files over 200 columns through `bcfgpu_sam -a AD,DP`, as BCF and as text, and a targets file from the cohort's
    own records -- by record index mod 5: its alleles as they are, REF plus a base the record lacks, its ALTs reversed, REF alone, no
    target -- with a few targets where no record lies."""
    build_host()
    d = tmp_path_factory.mktemp("cohort_als")
    G = os.path.join(golden_dir, "mpileup")
    ref = "".join(ln.strip() for ln in open(os.path.join(G, "mpileup.ref.fa")) if not ln.startswith(">"))
    files = []
    for s in range(70):
        files.append(str(d / ("c%02d.sam" % s)))
        _cohort_sam(files[-1], ref, "c%02d" % s, 1000 + s, 1000, 1200)
    bcf, vcf = str(d / "cohort.bcf"), str(d / "cohort.vcf")
    subprocess.check_call([SAM_EXE, "-a", "AD,DP", "-O", "u", "-o", bcf, "-f", os.path.join(G, "mpileup.ref.fa"), "-r", "17:1001-1200"] + files)
    subprocess.check_call([VIEW_EXE, "-O", "v", "-o", vcf, bcf])
    names = ["c%02d" % s for s in range(70)]
    (d / "reversed.txt").write_text("".join(n + "\n" for n in names[::-1]))
    (d / "three.txt").write_text("c41\nc03\nc69\n")
    (d / "groups.txt").write_text("".join("%s\t%s\n" % (n, "even" if i % 2 == 0 else "odd") for i, n in enumerate(names)))
    tab = ["17\t900\tA,C\n"]
    for i, r in enumerate(V.Vcf(vcf).recs):
        real = [a for a in r.alts if not a.startswith("<")]
        if i % 5 == 0:
            als = [r.ref] + real
        elif i % 5 == 1:
            lacks = [b for b in "ACGT" if b not in [r.ref[0].upper()] + [a.upper() for a in real]]
            als = [r.ref, lacks[0] + r.ref[1:] if lacks else r.ref + "A"]      # (all four bases seen: an insertion)
        elif i % 5 == 2:
            als = [r.ref] + real[::-1]
        elif i % 5 == 3:
            als = [r.ref]
        else:
            continue
        tab.append("%s\t%d\t%s\n" % (r.chrom, r.pos, ",".join(als)))
    tab += ["17\t1300\tG,T\n", "17\t1301\tGA,G\n"]
    (d / "targets.tab").write_text("".join(tab))
    return d, {"bcf": bcf, "text": vcf}


@pytest.mark.parametrize("kind", ["text", "bcf"])
@pytest.mark.parametrize("args,n_smpl", [("-i", 70), ("-i -S {D}/reversed.txt", 70), ("-S {D}/three.txt", 3), ("-G {D}/groups.txt --group-samples-tag AD", 70)])
def test_device_alleles_on_a_cohort_past_one_wavefront(cohort, args, n_smpl, kind):
    """The host route is the reference here (the nine goldens pin it)."""
    d, inputs = cohort
    cmd = [CALL_EXE, "-m", "-A", "-C", "alleles", "-T", str(d / "targets.tab")] + args.format(D=str(d)).split() + [inputs[kind]]
    seen, out = None, {}
    for mode in ("v", "u"):
        plain, dev = run(cmd, mode=mode), run(cmd, [IN_OPT[kind], OPT], mode)
        assert plain.stderr == b"" and dev.stdout == plain.stdout, mode
        n, m = counts(ALS_LINE, dev.stderr)
        assert n > 0 and m > 0 and n + m == decoded(kind, dev.stderr) and (seen is None or seen == (n, m))
        seen, out[mode] = (n, m), plain.stdout
    recs = [ln.split("\t") for ln in as_text(out["u"]).splitlines() if ln and not ln.startswith("#")]
    assert all(len(r) == 9 + n_smpl for r in recs)
    called = [r for r in recs if r[8] != "GT"]
    assert 100 < len(called) <= n + m and ("-i" in args) == (len(called) < len(recs))
    for mode, opts in (("u", ["--device-records", "--device-keys"]), ("v", ["--device-text"])):
        assert run(cmd, [IN_OPT[kind], OPT] + opts, mode).stdout == out[mode]


def test_device_alleles_does_nothing_without_an_input_option_in_effect(golden_dir, tmp_path):
    """Without an input option, with --device-input on text and with --device-parse on BCF: the same bytes, and no line of --timing
    counts a record."""
    build_host()
    G = os.path.join(golden_dir, "call")
    vcf = os.path.join(G, "mpileup.2.vcf")
    bcf = to_bcf(vcf, str(tmp_path / "in.bcf"))
    tab = ["-m", "-A", "-C", "alleles", "-T", os.path.join(G, "mpileup.2.tab")]
    plain = {path: run([CALL_EXE] + tab + [path]) for path in (vcf, bcf)}
    assert plain[vcf].stdout == plain[bcf].stdout and n_records(plain[vcf].stdout.decode()) > 0
    for path, opts in ((vcf, [OPT]), (bcf, [OPT]), (vcf, [OPT, "--device-input"]), (bcf, [OPT, "--device-parse"])):
        dev = run([CALL_EXE] + tab + [path], opts)
        assert plain[path].stderr == b"" and dev.stdout == plain[path].stdout
        assert counts(ALS_LINE, dev.stderr) == (0, 0) and device_count(dev.stderr) == 0
        assert b"device parse: " not in dev.stderr or parse_count(dev.stderr) == 0


def test_device_alleles_does_nothing_without_constrained_alleles(golden_dir, tmp_path):
    """Without -C alleles the input option acts as ever, and the option's line counts nothing."""
    build_host()
    G = os.path.join(golden_dir, "call")
    vcf = os.path.join(G, "mpileup.2.vcf")
    for kind, path in (("text", vcf), ("bcf", to_bcf(vcf, str(tmp_path / "in.bcf")))):
        cmd = [CALL_EXE, "-v", path]
        plain, dev = run(cmd), run(cmd, [OPT, IN_OPT[kind]])
        assert dev.stdout == plain.stdout and counts(ALS_LINE, dev.stderr) == (0, 0)
        assert decoded(kind, dev.stderr) > 0
