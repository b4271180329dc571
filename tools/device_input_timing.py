"""What `bcfgpu_call --device-input` does to the caller's input side at cohort scale: the PL and AD planes made on the device
from the records' bytes (bcfgpu_call_decode_bcf), the sample columns turned into text only for the records that are written,
against the text route (every value of every sample of every record printed by the BCF reader and parsed back by the driver).

    python tools/device_input_timing.py [--samples 256] [--depth 30] [--columns 16384] [--tile 4096] [--repeats 5]
                                        [--out profiles/device_input.txt] [--keep DIR]

It writes the seeded cohort of tools/device_records_timing.py, turns it into one uncompressed BCF with
`bcfgpu_sam -a AD,DP -O u`, once, and then runs `bcfgpu_call -mv --timing -O u` on that file without and with --device-input,
alternating, --repeats times each after one warm-up run of each; then the same pair without -v, where every record is written
(the lazy text saves nothing there: only the planes' part shows).  Every --timing line, the medians and the spreads (largest
- smallest) go to --out.  The baseline is the same binary without the option, in the same visit.  The two outputs must be
byte-equal; the tool fails if they are not, and it fails without a GPU."""
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
from device_records_timing import RLEN, SAM_EXE, write_cohort  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL_EXE = os.path.join(ROOT, "host", "bcfgpu_call")
FIELDS = ("reading records", "building the planes on the host", "uploads and device stages", "writing records")


def run(cmd):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    if p.returncode:
        raise SystemExit("%s failed (%d):\n%s" % (" ".join(cmd[:6]), p.returncode, p.stderr.decode()[-2000:]))
    err = p.stderr.decode()
    line = next(ln for ln in err.splitlines() if "seconds: reading records" in ln)
    vals = [float(re.search(re.escape(k) + r" ([0-9.]+)", line).group(1)) for k in FIELDS]
    dev = re.search(r"device input: (\d+) records", err)
    return dict(wall=wall, line=line, vals=vals, n_dev=int(dev.group(1)), sha=hashlib.sha256(p.stdout).hexdigest(), nbytes=len(p.stdout))


def compare(title, args, bcf, repeats, lines):
    """One pair of commands, alternating; appends its part of the report; False when the outputs differ."""
    base = [CALL_EXE] + args + ["--timing", "-O", "u", bcf]
    with_opt = base[:1] + ["--device-input"] + base[1:]
    runs = {"text": [], "device": []}
    run(base), run(with_opt)                                                       # warm-up: the page cache, the code objects
    for _ in range(max(1, repeats)):                                               # alternating, in one visit
        runs["text"].append(run(base))
        runs["device"].append(run(with_opt))
    shas = {r["sha"] for rs in runs.values() for r in rs}
    lines.append(title)
    lines.append("-" * len(title))
    lines.append("Output: %d bytes of uncompressed BCF to a pipe; %d records' planes decoded on the device with the option, %d without." %
                 (runs["text"][0]["nbytes"], runs["device"][0]["n_dev"], runs["text"][0]["n_dev"]))
    for kind in ("text", "device"):
        lines.append("%s route (%s):" % (kind, "the parent commit's path: no option" if kind == "text" else "--device-input"))
        for r in runs[kind]:
            lines.append("    %s    [wall %.3f]" % (r["line"], r["wall"]))
    lines.append("")
    lines.append("%-34s %26s %26s %12s %8s" % ("seconds", "text route: median (spread)", "device: median (spread)", "difference", "a gain?"))
    for i, k in enumerate(FIELDS + ("wall time of the process",)):
        row, med, spread = [], [], []
        for kind in ("text", "device"):
            v = [r["vals"][i] if i < len(FIELDS) else r["wall"] for r in runs[kind]]
            med.append(statistics.median(v))
            spread.append(max(v) - min(v))
            row.append("%.3f (%.3f)" % (med[-1], spread[-1]))
        diff = med[1] - med[0]                                                     # a gain only past both spreads
        lines.append("%-34s %26s %26s %+12.3f %8s" % (k, row[0], row[1], diff, "yes" if -diff > max(spread) else "slower" if diff > max(spread) else "no"))
    lines.append("")
    lines.append("outputs byte-equal in every run: %s (sha256 %s)" % ("yes" if len(shas) == 1 else "NO", sorted(shas)[0][:16]))
    lines.append("")
    return len(shas) == 1 and runs["device"][0]["n_dev"] > 0 and runs["text"][0]["n_dev"] == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--columns", type=int, default=16384)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_input.txt"))
    ap.add_argument("--keep", metavar="DIR", help="write the SAM files and the BCF here and leave them")
    a = ap.parse_args()
    tmp = None if a.keep else tempfile.TemporaryDirectory(prefix="bcfgpu_cohort_")
    d = a.keep or tmp.name
    os.makedirs(d, exist_ok=True)
    ref = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(a.seed).integers(0, 4, a.columns + RLEN)].tobytes().decode()
    REF = os.path.join(d, "ref.fa")
    with open(REF, "w") as f:
        f.write(">17\n" + "\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + "\n")
    files, n_reads = write_cohort(d, ref, a.samples, a.depth, a.columns, a.seed)
    bcf = os.path.join(d, "cohort.bcf")
    subprocess.check_call([SAM_EXE, "-O", "u", "-o", bcf, "-a", "AD,DP", "--tile", str(a.tile), "-f", REF, "-r", "17:1-%d" % a.columns] + files)
    for f in files:                                                                # (the BCF alone is read from here on)
        if not a.keep:
            os.remove(f)
    lines = []
    lines.append("bcfgpu_call --timing -O u, without and with --device-input: tools/device_input_timing.py, one MI355X, one GPU visit")
    lines.append("=" * 118)
    lines.append("")
    lines.append("Input: %d single-sample SAM files, %.0fx, reads of %d bases over 17:1-%d of a random reference (seed %d): %d reads," %
                 (a.samples, a.depth, RLEN, a.columns, a.seed, n_reads))
    lines.append("written once as uncompressed BCF by bcfgpu_sam -a AD,DP --tile %d: %d bytes." % (a.tile, os.path.getsize(bcf)))
    lines.append("One warm-up run of each, then %d runs of each, alternating; seconds as --timing prints them, and the process's wall time." % max(1, a.repeats))
    lines.append("\"a gain?\": yes / slower only where the medians differ by more than both spreads.")
    lines.append("")
    ok = compare("bcfgpu_call -mv (only the variant records are written)", ["-m", "-v"], bcf, a.repeats, lines)
    ok = compare("bcfgpu_call -m (every record is written: the lazy text saves nothing)", ["-m"], bcf, a.repeats, lines) and ok
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    if tmp:
        tmp.cleanup()
    if not ok:
        raise SystemExit("the outputs with and without --device-input differ, or the option did not take effect")


if __name__ == "__main__":
    main()
