"""`bcfgpu_sam --device-text`: with text output (-O v|z) the sample columns of every SNP and indel record are formatted on the
device (bcfgpu_mplp_encode_vcf) and the host downloads bytes and offsets instead of the planes.  The output must be the output
without the option, byte for byte, and the reference's goldens, whole files: every tile size, every FORMAT key, gVCF blocks
(which stay on the host path), --prefetch, region shards, -B, -C, more samples than a wavefront has lanes.  --timing's extra
line proves that the path ran; with BCF output the option does nothing, and it goes together with --device-records."""
import gzip
import os
import re
import subprocess

import pytest

from tests.test_c_host import SAM_EXE, TILE_CASES, _tile_cmd, build_host, whole_file_checks
from tests.test_c_host_device_records import _cohort_sam

pytestmark = pytest.mark.gpu

OPT = "--device-text"


def _run(cmd, extra):
    return subprocess.run(cmd[:1] + extra + cmd[1:], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _same_with_and_without(cmd, modes=("v", "z")):
    """cmd -O v (and -O z, compared after decompression) with and without the option: the same bytes; returns the text."""
    out = None
    for mode in modes:
        plain, dev = _run(cmd, ["-O", mode]).stdout, _run(cmd, [OPT, "-O", mode]).stdout
        if mode == "z":
            assert dev[:2] == b"\x1f\x8b"
            plain, dev = gzip.decompress(plain), gzip.decompress(dev)
        assert dev == plain, mode
        assert out is None or out == plain
        out = plain
    return out


def _device_count(stderr):
    m = re.search(rb"device text: (\d+) records with their sample columns formatted on the device", stderr)
    assert m, stderr
    return int(m.group(1))


@pytest.mark.parametrize("tile", [64, 512])
@pytest.mark.parametrize("goldf", sorted(TILE_CASES))
def test_device_text_on_every_tiled_golden(golden_dir, goldf, tile):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    cmd = _tile_cmd(G, goldf, ["--tile", str(tile)])
    whole_file_checks(cmd[:1] + [OPT] + cmd[1:], os.path.join(G, goldf))
    assert len(_same_with_and_without(cmd)) > 1000


@pytest.mark.parametrize("tags,goldf", [("DP,DPR,DV,DP4,INFO/DPR,SP", "mpileup.4.out"),
                                        ("DP,AD,ADF,ADR,SP,INFO/AD,INFO/ADF,INFO/ADR", "mpileup.5.out")])
def test_device_text_with_the_goldens_tag_sets(golden_dir, tags, goldf):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    cmd = [SAM_EXE, "-a", tags, os.path.join(G, "mpileup.ref.fa"), "17", "100", "600"] + [os.path.join(G, "mpileup.%d.sam" % i) for i in (1, 2, 3)]
    whole_file_checks(cmd[:1] + [OPT] + cmd[1:], os.path.join(G, goldf))
    _same_with_and_without(cmd)


def test_device_text_scr_and_qs_from_a_bam(golden_dir):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    tail = [os.path.join(G, "mpileup-SCR.fa"), "1", "1", "150", os.path.join(G, "mpileup-SCR.bam")]
    whole_file_checks([SAM_EXE, OPT, "-a", "INFO/SCR,FMT/SCR"] + tail, os.path.join(G, "mpileup-SCR.out"))
    out = _same_with_and_without([SAM_EXE, "-a", "SCR,QS"] + tail)
    assert b"\tPL:SCR:QS\t" in out


@pytest.mark.parametrize("extra", [["--prefetch", "--tile", "64"], ["--gpus", "2", "--tile", "128"], ["-B", "--tile", "64"], ["-C", "50", "--tile", "256"]],
                         ids=lambda e: "".join(e))
def test_device_text_with_prefetch_shards_and_without_baq(golden_dir, extra):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    out = _same_with_and_without(_tile_cmd(G, "mpileup.11.out", extra), modes=("v",))
    assert len(out) > 10000 and out.count(b"INDEL") > 0


@pytest.mark.parametrize("tile", [37, 128])
def test_device_text_leaves_gvcf_blocks_to_the_host(golden_dir, tile):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    cmd = _tile_cmd(G, "mpileup.6.out", ["--tile", str(tile)])                 # --gvcf 0,2,5
    whole_file_checks(cmd[:1] + [OPT] + cmd[1:], os.path.join(G, "mpileup.6.out"))
    _same_with_and_without(cmd)
    _same_with_and_without(cmd[:1] + ["--prefetch"] + cmd[1:], modes=("v",))


def test_device_text_past_one_wavefront_of_samples(golden_dir, tmp_path):
    """70 single-sample files over 200 columns: more samples than a wavefront has lanes, PL of up to five alleles."""
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    ref = "".join(ln.strip() for ln in open(os.path.join(G, "mpileup.ref.fa")) if not ln.startswith(">"))
    files = []
    for s in range(70):
        files.append(str(tmp_path / ("c%02d.sam" % s)))
        _cohort_sam(files[-1], ref, "c%02d" % s, 1000 + s, 1000, 1200)
    cmd = [SAM_EXE, "-a", "AD,DP,SP", "--tile", "128", "-f", os.path.join(G, "mpileup.ref.fa"), "-r", "17:1001-1200"] + files
    out = _same_with_and_without(cmd).decode()
    recs = [ln.split("\t") for ln in out.splitlines() if not ln.startswith("#")]
    assert len(recs) >= 200 and all(len(r) == 9 + 70 for r in recs)
    assert max(len(r[4].split(",")) for r in recs) >= 3


def test_device_text_does_nothing_with_bcf_output_and_goes_with_device_records(golden_dir):
    """-O u: the plain bytes, 0 records counted.  Both options together: each acts on its own output modes."""
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    cmd = _tile_cmd(G, "mpileup.2.out", ["--tile", "256"])
    plain = {m: _run(cmd, ["-O", m]).stdout for m in ("v", "z", "u", "b")}
    p = _run(cmd, [OPT, "--timing", "-O", "u"])
    assert p.stdout == plain["u"] and _device_count(p.stderr) == 0
    n_rec = sum(1 for ln in plain["v"].splitlines() if not ln.startswith(b"#"))
    for m in ("v", "z", "u", "b"):
        q = _run(cmd, [OPT, "--device-records", "--timing", "-O", m])
        if m == "z":
            assert gzip.decompress(q.stdout) == gzip.decompress(plain[m]) == plain["v"]
        else:
            assert q.stdout == plain[m], m
        n_text = _device_count(q.stderr)
        n_bcf = int(re.search(rb"device records: (\d+) records", q.stderr).group(1))
        assert (n_text, n_bcf) == ((n_rec, 0) if m in "vz" else (0, n_rec)), m


def test_timing_line_counts_the_records_formatted_on_the_device(golden_dir):
    """--timing: one more stderr line with the number of records whose sample columns came from the device -- every record that
    is not a gVCF block line.  Without the option stderr has no such line and is otherwise the same lines."""
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    for goldf in ("mpileup.11.out", "mpileup.6.out"):
        cmd = _tile_cmd(G, goldf, ["--tile", "128"])
        p = _run(cmd, [OPT, "--timing", "-O", "v"])
        assert b"writing records" in p.stderr
        recs = [ln for ln in p.stdout.decode().splitlines() if not ln.startswith("#")]
        n_plain = sum(1 for ln in recs if "MinDP=" not in ln.split("\t")[7])
        assert _device_count(p.stderr) == n_plain > 0
        assert (n_plain < len(recs)) == (goldf == "mpileup.6.out")
        q = _run(cmd, ["--timing", "-O", "v"])
        assert q.stdout == p.stdout and b"device text" not in q.stderr
        # the lines without the option are the lines with it but for the last one (the seconds in them vary from run to run)
        strip = lambda err: [re.sub(rb"\d+\.\d+", b"#", ln) for ln in err.splitlines()]
        assert strip(p.stderr)[:-1] == strip(q.stderr) and strip(p.stderr)[-1].startswith(b"[bcfgpu_sam] device text: ")
        assert b"device records: 0 records" in q.stderr
        r = _run(cmd, ["-O", "v"])
        assert r.stdout == p.stdout and b"device text" not in r.stderr and b"device records" not in r.stderr


def test_the_option_is_in_the_usage_text():
    build_host()
    p = subprocess.run([SAM_EXE], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 2 and b"[--device-text]" in p.stderr
