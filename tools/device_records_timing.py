"""What `bcfgpu_sam --device-records` does to the writer at cohort scale: the per-sample part of every record encoded on the
device (bcfgpu_mplp_encode_bcf) against the host path (planes to the host, print_record's transposition, the writer's range
scan and narrowing).

    python tools/device_records_timing.py [--samples 256] [--depth 30] [--columns 16384] [--tile 4096] [--repeats 5]
                                          [--out profiles/device_records.txt] [--keep DIR]

It writes a seeded reference (one contig "17" of --columns + 150 random bases) and a seeded cohort of single-sample SAM files
over its first --columns positions (reads of 150 bases, a mismatch rate of 1 %, a shared SNP every 500 bases that three samples
in ten carry), then runs
`bcfgpu_sam --timing -O u` without and with --device-records, alternating, --repeats times each after one warm-up run of
each, and writes every --timing line, the medians and the spreads (largest - smallest) to --out.  The baseline is the same
binary without the option, in the same visit.  The two outputs must be byte-equal; the tool fails if they are not, and it
fails without a GPU (bcfgpu_sam has no CPU path)."""
import argparse
import hashlib
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAM_EXE = os.path.join(ROOT, "host", "bcfgpu_sam")
RLEN = 150
FIELDS = ("reading and parsing the files", "tile pools", "device stages", "writing records", "waiting in bcfgpu_pool_adopt")


def write_cohort(d, ref, n_smpl, depth, columns, seed):
    """n_smpl SAM files, one sample each, `depth` reads deep over [0, columns) of contig 17."""
    codes = np.frombuffer(ref.upper().encode(), np.uint8)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    rng0 = np.random.default_rng(seed)
    snp_pos = np.sort(rng0.choice(np.arange(200, columns - 200), size=max(1, columns // 500), replace=False))     # shared by the cohort
    snp_alt = acgt[rng0.integers(0, 4, len(snp_pos))]
    files, n_reads = [], 0
    for s in range(n_smpl):
        rng = np.random.default_rng(seed * 100003 + s)
        n = int(columns * depth / RLEN)
        pos = np.sort(rng.integers(0, max(1, columns - RLEN), n))
        seq = codes[pos[:, None] + np.arange(RLEN)[None, :]].copy()
        carrier = rng.random(len(snp_pos)) < 0.3                                   # this sample carries the SNP (on all its reads)
        for p, a in zip(snp_pos[carrier], snp_alt[carrier]):
            hit = (pos <= p) & (p < pos + RLEN)
            seq[hit, p - pos[hit]] = a
        err = rng.random(seq.shape) < 0.01
        seq[err] = acgt[rng.integers(0, 4, int(err.sum()))]
        qual = (33 + rng.integers(15, 41, seq.shape)).astype(np.uint8)
        flag = 16 * rng.integers(0, 2, n)
        mapq = rng.choice([20, 40, 60], n)
        sb, qb = seq.tobytes().decode(), qual.tobytes().decode()
        name = "s%04d" % s
        path = os.path.join(d, name + ".sam")
        with open(path, "w") as f:
            f.write("@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:17\tLN:%d\n@RG\tID:%s\tSM:%s\n" % (len(ref), name, name))
            f.write("".join("r%d\t%d\t17\t%d\t%d\t%dM\t*\t0\t0\t%s\t%s\tRG:Z:%s\n" %
                            (i, flag[i], pos[i] + 1, mapq[i], RLEN, sb[i * RLEN:(i + 1) * RLEN], qb[i * RLEN:(i + 1) * RLEN], name) for i in range(n)))
        files.append(path)
        n_reads += n
    return files, n_reads


def run(cmd):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    if p.returncode:
        raise SystemExit("%s failed (%d):\n%s" % (" ".join(cmd[:6]), p.returncode, p.stderr.decode()[-2000:]))
    err = p.stderr.decode()
    line = next(ln for ln in err.splitlines() if "seconds: reading and parsing" in ln)
    vals = [float(re.search(re.escape(k) + r" ([0-9.]+)", line).group(1)) for k in FIELDS]
    dev = re.search(r"device records: (\d+) records", err)
    return dict(wall=wall, line=line, vals=vals, n_dev=int(dev.group(1)) if dev else -1, sha=hashlib.sha256(p.stdout).hexdigest(), nbytes=len(p.stdout))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--columns", type=int, default=16384)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--prefetch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_records.txt"))
    ap.add_argument("--keep", metavar="DIR", help="write the SAM files here and leave them")
    a = ap.parse_args()
    tmp = None if a.keep else tempfile.TemporaryDirectory(prefix="bcfgpu_cohort_")
    d = a.keep or tmp.name
    os.makedirs(d, exist_ok=True)
    ref = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(a.seed).integers(0, 4, a.columns + RLEN)].tobytes().decode()
    REF = os.path.join(d, "ref.fa")
    with open(REF, "w") as f:
        f.write(">17\n" + "\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + "\n")
    t0 = time.perf_counter()
    files, n_reads = write_cohort(d, ref, a.samples, a.depth, a.columns, a.seed)
    t_gen = time.perf_counter() - t0
    base = [SAM_EXE, "--timing", "-O", "u", "-a", "AD,DP", "--tile", str(a.tile)] + (["--prefetch"] if a.prefetch else []) + \
           ["-f", REF, "-r", "17:1-%d" % a.columns] + files
    with_opt = base[:1] + ["--device-records"] + base[1:]
    runs = {"host": [], "device": []}
    run(base), run(with_opt)                                                       # warm-up: the page cache, the code objects
    for _ in range(max(1, a.repeats)):                                             # alternating, in one visit
        runs["host"].append(run(base))
        runs["device"].append(run(with_opt))
    shas = {r["sha"] for rs in runs.values() for r in rs}
    lines = []
    lines.append("bcfgpu_sam --timing -O u, without and with --device-records: tools/device_records_timing.py, one MI355X, one GPU visit")
    lines.append("=" * 118)
    lines.append("")
    lines.append("Cohort: %d single-sample SAM files, %.0fx, reads of %d bases over 17:1-%d of a random reference (seed %d): %d reads," %
                 (a.samples, a.depth, RLEN, a.columns, a.seed, n_reads))
    lines.append("-a AD,DP, --tile %d%s; written in %.1f s.  Output: %d bytes of uncompressed BCF to a pipe, %d records with a block from the device." %
                 (a.tile, ", --prefetch" if a.prefetch else "", t_gen, runs["host"][0]["nbytes"], runs["device"][0]["n_dev"]))
    lines.append("One warm-up run of each, then %d runs of each, alternating; seconds as --timing prints them, and the process's wall time." % len(runs["host"]))
    lines.append("")
    for kind in ("host", "device"):
        lines.append("%s path (%s):" % (kind, "the parent commit's path: no option" if kind == "host" else "--device-records"))
        for r in runs[kind]:
            lines.append("    %s    [wall %.3f]" % (r["line"], r["wall"]))
    lines.append("")
    lines.append("%-32s %26s %26s %12s" % ("seconds", "host path: median (spread)", "device: median (spread)", "difference"))
    med = {}
    for i, k in enumerate(FIELDS + ("wall time of the process",)):
        row = []
        for kind in ("host", "device"):
            v = [r["vals"][i] if i < len(FIELDS) else r["wall"] for r in runs[kind]]
            med[(kind, k)] = statistics.median(v)
            row.append("%.3f (%.3f)" % (statistics.median(v), max(v) - min(v)))
        lines.append("%-32s %26s %26s %+12.3f" % (k, row[0], row[1], med[("device", k)] - med[("host", k)]))
    lines.append("")
    lines.append("outputs byte-equal in every run: %s (sha256 %s)" % ("yes" if len(shas) == 1 else "NO", sorted(shas)[0][:16]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    if tmp:
        tmp.cleanup()
    if len(shas) != 1:
        raise SystemExit("the outputs with and without --device-records differ")
    if runs["device"][0]["n_dev"] <= 0:
        raise SystemExit("--device-records encoded no record on the device")


if __name__ == "__main__":
    main()
