"""What `bcfgpu_sam --device-text` does to a VCF text run at cohort scale: the sample columns of every record formatted on the
device (bcfgpu_mplp_encode_vcf) against the host path (planes to the host, print_record's transposition, the writer's digit
loop).

    python tools/device_text_timing.py [--samples 256] [--depth 30] [--columns 16384] [--tile 4096] [--repeats 5]
                                       [--out profiles/device_text.txt] [--keep DIR]

The cohort is that of tools/device_records_timing.py (its writer is imported: a seeded reference and seeded single-sample SAM
files).  `bcfgpu_sam --timing -O v` writes to a pipe, without and with --device-text, alternating, --repeats times each after
one warm-up run of each; every --timing line, the medians and the spreads (largest - smallest) of "device stages", "writing
records" and the process's wall time go to --out.  The baseline is the same binary without the option, in the same visit, and
no ratio is expected in advance: the verdict line claims a gain (or a loss) only where the medians differ by more than both
spreads.  The outputs must be byte-equal in every run; the tool fails if they are not, and it fails without a GPU
(bcfgpu_sam has no CPU path)."""
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from device_records_timing import FIELDS, RLEN, ROOT, SAM_EXE, write_cohort  # noqa: E402

REPORTED = ("device stages", "writing records")


def run(cmd):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    if p.returncode:
        raise SystemExit("%s failed (%d):\n%s" % (" ".join(cmd[:6]), p.returncode, p.stderr.decode()[-2000:]))
    err = p.stderr.decode()
    line = next(ln for ln in err.splitlines() if "seconds: reading and parsing" in ln)
    vals = {k: float(re.search(re.escape(k) + r" ([0-9.]+)", line).group(1)) for k in FIELDS}
    dev = re.search(r"device text: (\d+) records", err)
    return dict(wall=wall, line=line, vals=vals, n_dev=int(dev.group(1)) if dev else -1, sha=hashlib.sha256(p.stdout).hexdigest(), nbytes=len(p.stdout))


def verdict(name, host, dev):
    """A difference is claimed only where the medians differ by more than both spreads."""
    mh, md = statistics.median(host), statistics.median(dev)
    sh, sd = max(host) - min(host), max(dev) - min(dev)
    if abs(md - mh) > max(sh, sd):
        return "%s: %s with --device-text (%.3f -> %.3f s, the difference exceeds both spreads)" % (name, "less" if md < mh else "MORE", mh, md)
    return "%s: no difference claimed (%.3f vs %.3f s, within the spreads %.3f and %.3f)" % (name, mh, md, sh, sd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--columns", type=int, default=16384)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--prefetch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_text.txt"))
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
    base = [SAM_EXE, "--timing", "-O", "v", "-a", "AD,DP", "--tile", str(a.tile)] + (["--prefetch"] if a.prefetch else []) + \
           ["-f", REF, "-r", "17:1-%d" % a.columns] + files
    with_opt = base[:1] + ["--device-text"] + base[1:]
    runs = {"host": [], "device": []}
    run(base), run(with_opt)                                                       # warm-up: the page cache, the code objects
    for _ in range(max(1, a.repeats)):                                             # alternating, in one visit
        runs["host"].append(run(base))
        runs["device"].append(run(with_opt))
    shas = {r["sha"] for rs in runs.values() for r in rs}
    lines = []
    lines.append("bcfgpu_sam --timing -O v, without and with --device-text: tools/device_text_timing.py, one MI355X, one GPU visit")
    lines.append("=" * 118)
    lines.append("")
    lines.append("Cohort: %d single-sample SAM files, %.0fx, reads of %d bases over 17:1-%d of a random reference (seed %d): %d reads," %
                 (a.samples, a.depth, RLEN, a.columns, a.seed, n_reads))
    lines.append("-a AD,DP, --tile %d%s; written in %.1f s.  Output: %d bytes of VCF text to a pipe, %d records with sample columns from the device." %
                 (a.tile, ", --prefetch" if a.prefetch else "", t_gen, runs["host"][0]["nbytes"], runs["device"][0]["n_dev"]))
    lines.append("One warm-up run of each, then %d runs of each, alternating; seconds as --timing prints them, and the process's wall time." % len(runs["host"]))
    lines.append("")
    for kind in ("host", "device"):
        lines.append("%s path (%s):" % (kind, "the parent commit's path: no option" if kind == "host" else "--device-text"))
        for r in runs[kind]:
            lines.append("    %s    [wall %.3f]" % (r["line"], r["wall"]))
    lines.append("")
    lines.append("%-32s %26s %26s %12s" % ("seconds", "host path: median (spread)", "device: median (spread)", "difference"))
    verdicts = []
    for k in REPORTED + ("wall time of the process",):
        v = {kind: [r["vals"][k] if k in FIELDS else r["wall"] for r in runs[kind]] for kind in runs}
        row = ["%.3f (%.3f)" % (statistics.median(v[kind]), max(v[kind]) - min(v[kind])) for kind in ("host", "device")]
        lines.append("%-32s %26s %26s %+12.3f" % (k, row[0], row[1], statistics.median(v["device"]) - statistics.median(v["host"])))
        verdicts.append(verdict(k, v["host"], v["device"]))
    lines.append("")
    lines.extend(verdicts)
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
        raise SystemExit("the outputs with and without --device-text differ")
    if runs["device"][0]["n_dev"] <= 0:
        raise SystemExit("--device-text formatted no record on the device")


if __name__ == "__main__":
    main()
