"""`bcfgpu_sam --device-records`: with BCF output the per-sample part of every SNP and indel record is encoded on the device
(bcfgpu_mplp_encode_bcf) and the host downloads bytes and offsets instead of the planes.  The output must be the output
without the option, byte for byte, and the reference's goldens, whole files: every tile size, every FORMAT key, gVCF blocks
(which stay on the host path), --prefetch, region shards, -B, -C, more samples than a wavefront has lanes.  --timing's extra
line proves that the path ran; with text output the option does nothing."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_c_host import SAM_EXE, TILE_CASES, VIEW_EXE, _tile_cmd, build_host, whole_file_checks

pytestmark = pytest.mark.gpu

OPT = "--device-records"


def _same_with_and_without(cmd, modes=("u", "b")):
    """cmd -O u (and -O b) with and without the option: the same bytes on stdout; returns the -O u bytes."""
    out = None
    for mode in modes:
        plain = subprocess.run(cmd[:1] + ["-O", mode] + cmd[1:], check=True, stdout=subprocess.PIPE).stdout
        dev = subprocess.run(cmd[:1] + [OPT, "-O", mode] + cmd[1:], check=True, stdout=subprocess.PIPE).stdout
        assert dev == plain, mode
        out = out or plain
    return out


def _device_count(stderr):
    m = re.search(rb"device records: (\d+) records", stderr)
    assert m, stderr
    return int(m.group(1))


@pytest.mark.parametrize("tile", [64, 512])
@pytest.mark.parametrize("goldf", sorted(TILE_CASES))
def test_device_records_on_every_tiled_golden(golden_dir, goldf, tile):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    cmd = _tile_cmd(G, goldf, ["--tile", str(tile)])
    whole_file_checks(cmd[:1] + [OPT] + cmd[1:], os.path.join(G, goldf))
    assert len(_same_with_and_without(cmd)) > 1000


@pytest.mark.parametrize("tags,goldf", [("DP,DPR,DV,DP4,INFO/DPR,SP", "mpileup.4.out"),
                                        ("DP,AD,ADF,ADR,SP,INFO/AD,INFO/ADF,INFO/ADR", "mpileup.5.out")])
def test_device_records_with_the_goldens_tag_sets(golden_dir, tags, goldf):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    cmd = [SAM_EXE, "-a", tags, os.path.join(G, "mpileup.ref.fa"), "17", "100", "600"] + [os.path.join(G, "mpileup.%d.sam" % i) for i in (1, 2, 3)]
    whole_file_checks(cmd[:1] + [OPT] + cmd[1:], os.path.join(G, goldf))
    _same_with_and_without(cmd)


def test_device_records_scr_and_qs_from_a_bam(golden_dir):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    tail = [os.path.join(G, "mpileup-SCR.fa"), "1", "1", "150", os.path.join(G, "mpileup-SCR.bam")]
    whole_file_checks([SAM_EXE, OPT, "-a", "INFO/SCR,FMT/SCR"] + tail, os.path.join(G, "mpileup-SCR.out"))
    out = _same_with_and_without([SAM_EXE, "-a", "SCR,QS"] + tail)
    text = subprocess.run([VIEW_EXE, "-"], input=out, check=True, stdout=subprocess.PIPE).stdout.decode()
    assert "\tPL:SCR:QS\t" in text


@pytest.mark.parametrize("extra", [["--prefetch", "--tile", "64"], ["--gpus", "2", "--tile", "128"], ["-B", "--tile", "64"], ["-C", "50", "--tile", "256"],
                                   ["--prefetch", "--gpus", "2", "--tile", "128"]], ids=lambda e: "".join(e))
def test_device_records_with_prefetch_shards_and_without_baq(golden_dir, extra):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    out = _same_with_and_without(_tile_cmd(G, "mpileup.11.out", extra), modes=("u",))
    assert len(out) > 10000 and out.count(b"INDEL") > 0
    if "--gpus" in extra and "--prefetch" in extra:
        cmd = _tile_cmd(G, "mpileup.11.out", extra)
        whole_file_checks(cmd[:1] + [OPT] + cmd[1:], os.path.join(G, "mpileup.11.out"))


@pytest.mark.parametrize("tile", [37, 128])
def test_device_records_leave_gvcf_blocks_to_the_host(golden_dir, tile):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    cmd = _tile_cmd(G, "mpileup.6.out", ["--tile", str(tile)])                 # --gvcf 0,2,5
    whole_file_checks(cmd[:1] + [OPT] + cmd[1:], os.path.join(G, "mpileup.6.out"))
    _same_with_and_without(cmd)
    _same_with_and_without(cmd[:1] + ["--prefetch"] + cmd[1:], modes=("u",))


def _cohort_sam(path, ref, sample, seed, lo, hi, depth=5, rlen=60):
    """Reads of one sample over [lo, hi) of contig 17 at about `depth`: the reference's bases with a few mismatches."""
    rng = np.random.default_rng(seed)
    n = (hi - lo + rlen) * depth // rlen
    with open(path, "w") as f:
        f.write("@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:17\tLN:%d\n@RG\tID:%s\tSM:%s\n" % (len(ref), sample, sample))
        for i, pos in enumerate(sorted(int(x) for x in rng.integers(lo - rlen + 1, hi, n))):
            seq = list(ref[pos:pos + rlen])
            for k in np.flatnonzero(rng.random(rlen) < 0.02):
                seq[k] = "ACGT"[int(rng.integers(0, 4))]
            qual = "".join(chr(33 + int(q)) for q in rng.integers(15, 41, rlen))
            f.write("r%d\t%d\t17\t%d\t%d\t%dM\t*\t0\t0\t%s\t%s\tRG:Z:%s\n" % (i, 16 * int(rng.integers(0, 2)), pos + 1, int(rng.choice([20, 40, 60])),
                                                                          rlen, "".join(seq), qual, sample))


def test_device_records_past_one_wavefront_of_samples(golden_dir, tmp_path):
    """70 single-sample files over 200 columns: more samples than a wavefront has lanes, PL of up to five alleles."""
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    ref = "".join(ln.strip() for ln in open(os.path.join(G, "mpileup.ref.fa")) if not ln.startswith(">"))
    files = []
    for s in range(70):
        files.append(str(tmp_path / ("c%02d.sam" % s)))
        _cohort_sam(files[-1], ref, "c%02d" % s, 1000 + s, 1000, 1200)
    cmd = [SAM_EXE, "-a", "AD,DP,SP", "--tile", "128", "-f", os.path.join(G, "mpileup.ref.fa"), "-r", "17:1001-1200"] + files
    out = _same_with_and_without(cmd)
    text = subprocess.run([VIEW_EXE, "-"], input=out, check=True, stdout=subprocess.PIPE).stdout.decode()
    recs = [ln.split("\t") for ln in text.splitlines() if not ln.startswith("#")]
    assert len(recs) >= 200 and all(len(r) == 9 + 70 for r in recs)
    assert max(len(r[4].split(",")) for r in recs) >= 3


def test_timing_line_counts_the_records_encoded_on_the_device(golden_dir):
    """--timing: one more stderr line with the number of records whose block came from the device -- every record that is not
    a gVCF block line; 0 with text output, where the option changes nothing."""
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    for goldf in ("mpileup.11.out", "mpileup.6.out"):
        cmd = _tile_cmd(G, goldf, ["--tile", "128"])
        p = subprocess.run(cmd[:1] + [OPT, "--timing", "-O", "u"] + cmd[1:], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert b"writing records" in p.stderr
        text = subprocess.run([VIEW_EXE, "-"], input=p.stdout, check=True, stdout=subprocess.PIPE).stdout.decode()
        recs = [ln for ln in text.splitlines() if not ln.startswith("#")]
        n_plain = sum(1 for ln in recs if "MinDP=" not in ln.split("\t")[7])
        assert _device_count(p.stderr) == n_plain > 0
        assert (n_plain < len(recs)) == (goldf == "mpileup.6.out")
        q = subprocess.run(cmd[:1] + ["--timing", "-O", "u"] + cmd[1:], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert _device_count(q.stderr) == 0 and q.stdout == p.stdout
    cmd = _tile_cmd(G, "mpileup.2.out", ["--tile", "128"])
    v = subprocess.run(cmd[:1] + ["--timing", "-O", "v"] + cmd[1:], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    w = subprocess.run(cmd[:1] + [OPT, "--timing", "-O", "v"] + cmd[1:], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert w.stdout == v.stdout and _device_count(w.stderr) == 0
