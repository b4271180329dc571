"""What `bcfgpu_call --device-text` does to the writer on VCF text input at cohort scale: the sample columns of the records that are
written rewritten on the device from the input's own text (bcfgpu_call_rewrite_vcf), against the route `--device-parse -O v` takes
without it (the GT, PL and GQ planes downloaded, the record's columns copied and split at tabs, every column at ':', every Number=R
field at ',', and all of it printed again, on one host thread).

    python tools/device_call_rewrite_timing.py [--shapes 256x16384,1000x4096] [--depth 30] [--tile 4096] [--repeats 3]
                                               [--out profiles/device_call_rewrite.txt] [--keep DIR]

Per shape (samples x columns) the cohort is that of tools/device_records_timing.py, written as VCF text by `bcfgpu_sam -a AD,DP,SP
-O v`.  `bcfgpu_call -v -O v --device-parse --timing`, and the same without -v (every record written), reads that file without and
with --device-text, alternating, --repeats times each after one warm-up run of each.  The baseline is the run without the option: the parent commit's route.  Every --timing line, the
medians and the spreads (largest - smallest) of "writing records", "uploads and device stages", their sum and the process's wall time
go to --out, then the two kernels' times from one more run of the option's form under `rocprofv3 --kernel-trace --stats` (left out,
and said so, where rocprofv3 is not to be had).  No target is fixed; a gain (or a loss) is claimed only where the medians differ by
more than both spreads.  The outputs must be byte-equal in every run; the tool fails if they are not, and it fails without a GPU."""
import argparse
import csv
import glob
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from device_parse_timing import CALL_EXE, run  # noqa: E402
from device_records_timing import RLEN, ROOT, SAM_EXE, write_cohort  # noqa: E402

TAGS = "AD,DP,SP"
BOTH = "writing records + device stages"
REPORTED = ("writing records", "uploads and device stages", BOTH, "reading records", "wall time of the process")
KERNELS = ("callrw_size_kernel", "callrw_write_kernel", "vcfdec_index_kernel", "vcfdec_parse_kernel")


def text_counts(cmd):
    """(N, M) of the option's --timing line."""
    err = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, check=True).stderr.decode()
    m = re.search(r"device text: (\d+) records' sample columns formatted on the device, (\d+) on the host", err)
    return (int(m.group(1)), int(m.group(2))) if m else (0, 0)


def kernel_times(cmd, d):
    """{kernel: (calls, total ms)} of one run of cmd under rocprofv3, or a sentence why not."""
    if not shutil.which("rocprofv3"):
        return "rocprofv3 is not on the PATH: the kernels' times were not measured"
    out = os.path.join(d, "prof")
    p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "s", "--output-format", "csv", "--"] + cmd,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if p.returncode or not files:
        return "the run under rocprofv3 failed (%d): the kernels' times were not measured" % p.returncode
    got = {}
    for row in csv.DictReader(open(files[0])):
        for k in KERNELS:
            if k in row.get("Name", ""):
                got[k] = (int(row["Calls"]), float(row["TotalDurationNs"]) / 1e6)
    shutil.rmtree(out, ignore_errors=True)
    return got


def verdict(name, base, opt):
    mb, mo = statistics.median(base), statistics.median(opt)
    sb, so = max(base) - min(base), max(opt) - min(opt)
    if abs(mo - mb) > max(sb, so):
        return "%s: %s with --device-text (%.3f -> %.3f s, the difference exceeds both spreads)" % (name, "less" if mo < mb else "MORE", mb, mo)
    return "%s: no difference claimed (%.3f vs %.3f s, within the spreads %.3f and %.3f)" % (name, mb, mo, sb, so)


def one_shape(a, d, n_smpl, columns, lines):
    ref = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(a.seed).integers(0, 4, columns + RLEN)].tobytes().decode()
    REF = os.path.join(d, "ref.fa")
    with open(REF, "w") as f:
        f.write(">17\n" + "\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + "\n")
    files, n_reads = write_cohort(d, ref, n_smpl, a.depth, columns, a.seed)
    vcf = os.path.join(d, "cohort.vcf")
    subprocess.check_call([SAM_EXE, "-O", "v", "-a", TAGS, "--tile", str(a.tile), "-o", vcf, "-f", REF, "-r", "17:1-%d" % columns] + files)
    for f in files:
        os.remove(f)
    lines.append("Cohort: %d single-sample SAM files, %.0fx, reads of %d bases over 17:1-%d of a random reference (seed %d): %d reads," %
                 (n_smpl, a.depth, RLEN, columns, a.seed, n_reads))
    lines.append("as VCF text of bcfgpu_sam -a %s -O v: %d bytes." % (TAGS, os.path.getsize(vcf)))
    lines.append("")
    bad = compare(a, d, "bcfgpu_call -v (only the variant records are written)", ["-v"], vcf, lines)
    bad = compare(a, d, "bcfgpu_call (every record is written)", [], vcf, lines) or bad
    os.remove(vcf)
    return bad


def compare(a, d, title, args, vcf, lines):
    """One case in its two forms, alternating; appends its part of the report; a sentence when something is wrong."""
    base = [CALL_EXE] + args + ["-O", "v", "--device-parse", "--timing", vcf]
    with_opt = base[:1] + ["--device-text"] + base[1:]
    n_dev, n_host = text_counts(with_opt)                                          # (also the warm-up of that form)
    run(base)
    runs = {"parse": [], "text": []}
    for _ in range(max(3, a.repeats)):                                             # alternating, in one visit
        runs["parse"].append(run(base))
        runs["text"].append(run(with_opt))
    for rs in runs.values():
        for r in rs:
            r["vals"][BOTH] = r["vals"]["writing records"] + r["vals"]["uploads and device stages"]
    shas = {r["sha"] for rs in runs.values() for r in rs}
    lines.append(title)
    lines.append("-" * len(title))
    lines.append("Output: %d bytes of VCF text to a pipe; with --device-text %d records' sample columns rewritten on the device, %d on the host." %
                 (runs["parse"][0]["nbytes"], n_dev, n_host))
    lines.append("One warm-up run of each form, then %d runs of each, alternating; seconds as --timing prints them, and the process's wall time." % len(runs["parse"]))
    for kind, what in (("parse", "--device-parse: the parent commit's route, the baseline"), ("text", "--device-parse --device-text")):
        lines.append("%s:" % what)
        for r in runs[kind]:
            lines.append("    %s    [wall %.3f]" % (r["line"], r["wall"]))
    lines.append("")
    lines.append("%-40s %26s %26s %12s" % ("seconds", "baseline: median (spread)", "option: median (spread)", "difference"))
    verdicts = []
    for k in REPORTED:
        v = {kind: [r["vals"][k] for r in runs[kind]] for kind in runs}
        row = ["%.3f (%.3f)" % (statistics.median(v[kind]), max(v[kind]) - min(v[kind])) for kind in ("parse", "text")]
        lines.append("%-40s %26s %26s %+12.3f" % (k, row[0], row[1], statistics.median(v["text"]) - statistics.median(v["parse"])))
        verdicts.append(verdict(k, v["parse"], v["text"]))
    lines.append("")
    lines.extend(verdicts)
    lines.append("")
    kt = kernel_times([c for c in with_opt if c != "--timing"], d)
    if isinstance(kt, str):
        lines.append(kt)
    else:
        lines.append("One more run of the option's form under rocprofv3 --kernel-trace --stats: calls, total ms")
        for k in KERNELS:
            lines.append("    %-24s %s" % (k, "%6d %10.3f" % kt[k] if k in kt else "not launched"))
    lines.append("")
    lines.append("outputs byte-equal in every run: %s (sha256 %s)" % ("yes" if len(shas) == 1 else "NO", sorted(shas)[0][:16]))
    lines.append("")
    if len(shas) != 1:
        return "the outputs with and without --device-text differ"
    if n_dev <= 0 or n_host:
        return "--device-text rewrote no record on the device (or left some to the host)"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x16384,1000x4096", help="SAMPLESxCOLUMNS,...")
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3, help="runs of each form (at least 3)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_call_rewrite.txt"))
    ap.add_argument("--keep", metavar="DIR", help="work here instead of a temporary directory")
    a = ap.parse_args()
    tmp = None if a.keep else tempfile.TemporaryDirectory(prefix="bcfgpu_cohort_")
    d = a.keep or tmp.name
    os.makedirs(d, exist_ok=True)
    lines = ["bcfgpu_call -v -O v --device-parse --timing on VCF text, without and with --device-text: tools/device_call_rewrite_timing.py, one MI355X, one GPU visit",
             "=" * 150, ""]
    failures = []
    for shape in a.shapes.split(","):
        n_smpl, columns = (int(x) for x in shape.split("x"))
        bad = one_shape(a, d, n_smpl, columns, lines)
        if bad:
            failures.append("%s: %s" % (shape, bad))
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    if tmp:
        tmp.cleanup()
    if failures:
        raise SystemExit("; ".join(failures))


if __name__ == "__main__":
    main()
