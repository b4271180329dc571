"""What `bcfgpu_call --device-records` does to the caller's output side at cohort scale: GT, PL and GQ of the records that are
written encoded as BCF2 key blocks on the device (bcfgpu_call_encode_bcf) and downloaded as bytes, against the text route (the
gt, PL and GQ planes of every input record downloaded, every genotype and PL value printed, split again and parsed by the
writer, which then picks the integer type) -- alone and together with --device-input.

    python tools/device_call_records_timing.py [--samples 256] [--depth 30] [--columns 16384] [--tile 4096] [--repeats 5]
                                               [--out profiles/device_call_records.txt] [--keep DIR]

It writes the seeded cohort of tools/device_records_timing.py and turns it into uncompressed BCF with `bcfgpu_sam -O u`, once
with -a AD,DP (pass-through keys, whose blocks stay the host's) and once with the default FORMAT (PL alone: a written record
touches no per-sample data on the host).  On each file it runs `bcfgpu_call -m -v --timing -O u` and the same without -v, each
in four forms -- no option (the parent commit's route), --device-records, --device-input, both --, alternating, --repeats times
each after one warm-up run of each.  Every --timing line, the medians and the spreads (largest - smallest) go to --out.  The
baseline is the same binary without the option, in the same visit; a gain is claimed only where the medians differ by more
than both spreads.  All outputs of a case must be byte-equal; the tool fails if they are not, and it fails without a GPU."""
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
FORMS = (("text", []), ("records", ["--device-records"]), ("input", ["--device-input"]), ("both", ["--device-input", "--device-records"]))


def run(cmd):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    if p.returncode:
        raise SystemExit("%s failed (%d):\n%s" % (" ".join(cmd[:8]), p.returncode, p.stderr.decode()[-2000:]))
    err = p.stderr.decode()
    line = next(ln for ln in err.splitlines() if "seconds: reading records" in ln)
    vals = [float(re.search(re.escape(k) + r" ([0-9.]+)", line).group(1)) for k in FIELDS]
    n_rec = int(re.search(r"device records: (\d+) records", err).group(1))
    n_in = int(re.search(r"device input: (\d+) records", err).group(1))
    return dict(wall=wall, line=line, vals=vals, n_rec=n_rec, n_in=n_in, sha=hashlib.sha256(p.stdout).hexdigest(), nbytes=len(p.stdout))


def compare(title, args, bcf, repeats, lines):
    """One case in its four forms, alternating; appends its part of the report; False when the outputs differ."""
    cmds = {name: [CALL_EXE] + opts + args + ["--timing", "-O", "u", bcf] for name, opts in FORMS}
    runs = {name: [] for name, _ in FORMS}
    for name, _ in FORMS:                                                          # warm-up: the page cache, the code objects
        run(cmds[name])
    for _ in range(max(1, repeats)):                                               # alternating, in one visit
        for name, _ in FORMS:
            runs[name].append(run(cmds[name]))
    shas = {r["sha"] for rs in runs.values() for r in rs}
    lines.append(title)
    lines.append("-" * len(title))
    lines.append("Output: %d bytes of uncompressed BCF to a pipe; %d records' FORMAT blocks encoded on the device with --device-records, %d without." %
                 (runs["text"][0]["nbytes"], runs["records"][0]["n_rec"], runs["text"][0]["n_rec"]))
    for name, opts in FORMS:
        lines.append("%s (%s):" % (name, " ".join(opts) if opts else "the parent commit's route: no option"))
        for r in runs[name]:
            lines.append("    %s    [wall %.3f]" % (r["line"], r["wall"]))
    lines.append("")
    for base, other in (("text", "records"), ("input", "both")):                   # the option's effect without and with --device-input
        lines.append("%-34s %26s %26s %12s %8s" % ("seconds", "%s: median (spread)" % base, "%s: median (spread)" % other, "difference", "a gain?"))
        for i, k in enumerate(FIELDS + ("wall time of the process",)):
            row, med, spread = [], [], []
            for name in (base, other):
                v = [r["vals"][i] if i < len(FIELDS) else r["wall"] for r in runs[name]]
                med.append(statistics.median(v))
                spread.append(max(v) - min(v))
                row.append("%.3f (%.3f)" % (med[-1], spread[-1]))
            diff = med[1] - med[0]                                                 # a gain only past both spreads
            lines.append("%-34s %26s %26s %+12.3f %8s" % (k, row[0], row[1], diff, "yes" if -diff > max(spread) else "slower" if diff > max(spread) else "no"))
        lines.append("")
    lines.append("outputs byte-equal in every run of all four forms: %s (sha256 %s)" % ("yes" if len(shas) == 1 else "NO", sorted(shas)[0][:16]))
    lines.append("")
    took = all(runs[n][0]["n_rec"] > 0 for n in ("records", "both")) and all(runs[n][0]["n_rec"] == 0 for n in ("text", "input"))
    return len(shas) == 1 and took


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--columns", type=int, default=16384)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_call_records.txt"))
    ap.add_argument("--keep", metavar="DIR", help="write the SAM files and the BCF files here and leave them")
    a = ap.parse_args()
    tmp = None if a.keep else tempfile.TemporaryDirectory(prefix="bcfgpu_cohort_")
    d = a.keep or tmp.name
    os.makedirs(d, exist_ok=True)
    ref = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(a.seed).integers(0, 4, a.columns + RLEN)].tobytes().decode()
    REF = os.path.join(d, "ref.fa")
    with open(REF, "w") as f:
        f.write(">17\n" + "\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + "\n")
    files, n_reads = write_cohort(d, ref, a.samples, a.depth, a.columns, a.seed)
    bcfs = {}
    for name, tags in (("AD,DP", ["-a", "AD,DP"]), ("PL alone", [])):
        bcfs[name] = os.path.join(d, "cohort.%s.bcf" % ("ad" if tags else "pl"))
        subprocess.check_call([SAM_EXE, "-O", "u", "-o", bcfs[name]] + tags + ["--tile", str(a.tile), "-f", REF, "-r", "17:1-%d" % a.columns] + files)
    for f in files:                                                                # (the BCF files alone are read from here on)
        if not a.keep:
            os.remove(f)
    lines = []
    lines.append("bcfgpu_call --timing -O u, without and with --device-records: tools/device_call_records_timing.py, one MI355X, one GPU visit")
    lines.append("=" * 124)
    lines.append("")
    lines.append("Input: %d single-sample SAM files, %.0fx, reads of %d bases over 17:1-%d of a random reference (seed %d): %d reads," %
                 (a.samples, a.depth, RLEN, a.columns, a.seed, n_reads))
    lines.append("written once as uncompressed BCF by bcfgpu_sam --tile %d: %d bytes with -a AD,DP, %d bytes with the default FORMAT (PL alone)." %
                 (a.tile, os.path.getsize(bcfs["AD,DP"]), os.path.getsize(bcfs["PL alone"])))
    lines.append("One warm-up run of each form, then %d runs of each, alternating; seconds as --timing prints them, and the process's wall time." % max(1, a.repeats))
    lines.append("\"a gain?\": yes / slower only where the medians differ by more than both spreads.")
    lines.append("")
    ok = True
    for name in ("AD,DP", "PL alone"):
        ok = compare("input FORMAT %s: bcfgpu_call -m -v (only the variant records are written)" % name, ["-m", "-v"], bcfs[name], a.repeats, lines) and ok
        ok = compare("input FORMAT %s: bcfgpu_call -m (every record is written)" % name, ["-m"], bcfs[name], a.repeats, lines) and ok
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    if tmp:
        tmp.cleanup()
    if not ok:
        raise SystemExit("the outputs with and without --device-records differ, or the option did not take effect")


if __name__ == "__main__":
    main()
