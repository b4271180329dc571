"""What `bcfgpu_call --device-text` does to the writer at cohort scale: the sample columns of the records that are written formatted as
VCF text on the device from the call planes and the input's bytes (bcfgpu_call_encode_vcf), against the route `-O v` takes
without it (the GT, PL and GQ planes downloaded, the input's per-sample bytes turned into text, split per sample and key and
re-printed key by key with the Number=R trimming, on one host thread).

    python tools/device_call_text_timing.py [--samples 256] [--depth 30] [--columns 16384] [--tile 4096] [--repeats 5]
                                            [--out profiles/device_call_text.txt] [--keep DIR]

It writes the seeded cohort of tools/device_records_timing.py and turns it into uncompressed BCF with `bcfgpu_sam -O u -a
AD,ADF,ADR,DP,SP`.  On that file it runs `bcfgpu_call -m -v --timing -O v` and the same without -v in three forms -- no option,
--device-input (the parent's route for BCF input: the baseline), and --device-input --device-text --, alternating, --repeats times
each after one warm-up run of each.  Every --timing line, the medians and the spreads (largest - smallest) go to --out, and a short
table of "writing records" and "uploads and device stages" with the ratio baseline / option.  No target is fixed; a gain is claimed
only where the medians differ by more than both spreads.  All outputs of a case must be byte-equal; the tool fails if they are not,
and it fails without a GPU."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from device_call_records_timing import CALL_EXE, FIELDS, ROOT, run  # noqa: E402
from device_records_timing import RLEN, SAM_EXE, write_cohort  # noqa: E402

FORMS = (("plain", []), ("input", ["--device-input"]), ("text", ["--device-input", "--device-text"]))
TAGS = "AD,ADF,ADR,DP,SP"


def text_counts(cmd):
    """(N, M) of the option's --timing line."""
    err = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, check=True).stderr.decode()
    m = re.search(r"device text: (\d+) records' sample columns formatted on the device, (\d+) on the host", err)
    return (int(m.group(1)), int(m.group(2))) if m else (0, 0)


def compare(title, args, bcf, repeats, lines):
    """One case in its three forms, alternating; appends its part of the report; False when the outputs differ."""
    cmds = {name: [CALL_EXE] + opts + args + ["--timing", "-O", "v", bcf] for name, opts in FORMS}
    runs = {name: [] for name, _ in FORMS}
    n_dev, n_host = text_counts(cmds["text"])                                      # (also the warm-up of that form)
    for name in ("plain", "input"):                                                # warm-up: the page cache, the code objects
        run(cmds[name])
    for _ in range(max(1, repeats)):                                               # alternating, in one visit
        for name, _ in FORMS:
            runs[name].append(run(cmds[name]))
    shas = {r["sha"] for rs in runs.values() for r in rs}
    lines.append(title)
    lines.append("-" * len(title))
    lines.append("Output: %d bytes of VCF text to a pipe; with --device-text %d records' sample columns formatted on the device, %d on the host." %
                 (runs["plain"][0]["nbytes"], n_dev, n_host))
    for name, opts in FORMS:
        lines.append("%s (%s):" % (name, " ".join(opts) if opts else "no option"))
        for r in runs[name]:
            lines.append("    %s    [wall %.3f]" % (r["line"], r["wall"]))
    lines.append("")
    for base, other in (("input", "text"), ("plain", "text")):
        lines.append("%-34s %26s %26s %12s %8s %8s" % ("seconds", "%s: median (spread)" % base, "%s: median (spread)" % other, "difference", "ratio", "a gain?"))
        for i, k in enumerate(FIELDS + ("wall time of the process",)):
            row, med, spread = [], [], []
            for name in (base, other):
                v = [r["vals"][i] if i < len(FIELDS) else r["wall"] for r in runs[name]]
                med.append(statistics.median(v))
                spread.append(max(v) - min(v))
                row.append("%.3f (%.3f)" % (med[-1], spread[-1]))
            diff = med[1] - med[0]                                                 # a gain only past both spreads
            ratio = "%.2f" % (med[0] / med[1]) if med[1] > 0 else "-"
            lines.append("%-34s %26s %26s %+12.3f %8s %8s" % (k, row[0], row[1], diff, ratio, "yes" if -diff > max(spread) else "slower" if diff > max(spread) else "no"))
        lines.append("")
    lines.append("outputs byte-equal in every run of all three forms: %s (sha256 %s)" % ("yes" if len(shas) == 1 else "NO", sorted(shas)[0][:16]))
    lines.append("")
    return len(shas) == 1 and n_dev > 0 and n_host == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--columns", type=int, default=16384)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_call_text.txt"))
    ap.add_argument("--keep", metavar="DIR", help="write the SAM files and the BCF file here and leave them")
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
    subprocess.check_call([SAM_EXE, "-O", "u", "-o", bcf, "-a", TAGS, "--tile", str(a.tile), "-f", REF, "-r", "17:1-%d" % a.columns] + files)
    for f in files:                                                                # (the BCF file alone is read from here on)
        if not a.keep:
            os.remove(f)
    lines = []
    lines.append("bcfgpu_call --timing -O v, --device-input without and with --device-text: tools/device_call_text_timing.py, one MI355X, one GPU visit")
    lines.append("=" * 150)
    lines.append("")
    lines.append("Input: %d single-sample SAM files, %.0fx, reads of %d bases over 17:1-%d of a random reference (seed %d): %d reads," %
                 (a.samples, a.depth, RLEN, a.columns, a.seed, n_reads))
    lines.append("written once as uncompressed BCF by bcfgpu_sam --tile %d -a %s: %d bytes." % (a.tile, TAGS, os.path.getsize(bcf)))
    lines.append("One warm-up run of each form, then %d runs of each, alternating; seconds as --timing prints them, and the process's wall time." % max(1, a.repeats))
    lines.append("\"ratio\": the first form's median over the second's.  \"a gain?\": yes / slower only where the medians differ by more than both spreads.")
    lines.append("")
    ok = compare("input FORMAT PL,%s: bcfgpu_call -m -v (only the variant records are written)" % TAGS, ["-m", "-v"], bcf, a.repeats, lines)
    ok = compare("input FORMAT PL,%s: bcfgpu_call -m (every record is written)" % TAGS, ["-m"], bcf, a.repeats, lines) and ok
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    if tmp:
        tmp.cleanup()
    if not ok:
        raise SystemExit("the outputs with and without --device-text differ, or the option did not take effect")


if __name__ == "__main__":
    main()
