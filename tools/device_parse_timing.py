"""What `bcfgpu_call --device-parse` does to a run on VCF text input at cohort scale: the PL planes parsed on the device from the
sample columns' text (bcfgpu_call_decode_vcf) against the host path (every line split at all its tabs, every column at ':' and
',', one atoi a value, the int32 planes across PCIe).

    python tools/device_parse_timing.py [--shapes 256x16384,1000x4096] [--depth 30] [--tile 4096] [--repeats 5]
                                        [--out profiles/device_parse.txt] [--keep DIR]

Per shape (samples x columns) the cohort is that of tools/device_records_timing.py (its writer is imported: a seeded reference
and seeded single-sample SAM files), written as VCF text by `bcfgpu_sam -a AD,DP -O v`.  `bcfgpu_call -v --timing` reads that
file without and with --device-parse, alternating, --repeats times each after one warm-up run of each; every --timing line, the
medians and the spreads (largest - smallest) of "building the planes on the host", "uploads and device stages", their sum and
the process's wall time go to --out.  The baseline is the same binary without the option -- the parent commit's text route --
on the same input in the same visit, and no ratio is expected in advance: a verdict line claims a gain (or a loss) only where
the medians differ by more than the spread of the text route's runs (and of the option's).  The outputs must be byte-equal in
every run; the tool fails if they are not, and it fails without a GPU (the drivers have no CPU path)."""
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
from device_records_timing import RLEN, ROOT, SAM_EXE, write_cohort  # noqa: E402

CALL_EXE = os.path.join(ROOT, "host", "bcfgpu_call")
FIELDS = ("reading records", "building the planes on the host", "uploads and device stages", "writing records")
PLANES = "planes: host building + device stages"
REPORTED = ("building the planes on the host", "uploads and device stages", PLANES, "reading records", "wall time of the process")


def run(cmd):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    if p.returncode:
        raise SystemExit("%s failed (%d):\n%s" % (" ".join(cmd[:6]), p.returncode, p.stderr.decode()[-2000:]))
    err = p.stderr.decode()
    line = next(ln for ln in err.splitlines() if "seconds: reading records" in ln)
    vals = {k: float(re.search(re.escape(k) + r" ([0-9.]+)", line).group(1)) for k in FIELDS}
    vals[PLANES] = vals["building the planes on the host"] + vals["uploads and device stages"]
    vals["wall time of the process"] = wall
    dev = re.search(r"device parse: (\d+) records", err)
    return dict(line=line, wall=wall, vals=vals, n_dev=int(dev.group(1)) if dev else 0, sha=hashlib.sha256(p.stdout).hexdigest(), nbytes=len(p.stdout))


def verdict(name, host, dev):
    """A difference is claimed only where the medians differ by more than both spreads."""
    mh, md = statistics.median(host), statistics.median(dev)
    sh, sd = max(host) - min(host), max(dev) - min(dev)
    if abs(md - mh) > max(sh, sd):
        return "%s: %s with --device-parse (%.3f -> %.3f s, the difference exceeds both spreads)" % (name, "less" if md < mh else "MORE", mh, md)
    return "%s: no difference claimed (%.3f vs %.3f s, within the spreads %.3f and %.3f)" % (name, mh, md, sh, sd)


def one_shape(a, d, n_smpl, columns, lines):
    ref = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(a.seed).integers(0, 4, columns + RLEN)].tobytes().decode()
    REF = os.path.join(d, "ref.fa")
    with open(REF, "w") as f:
        f.write(">17\n" + "\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + "\n")
    files, n_reads = write_cohort(d, ref, n_smpl, a.depth, columns, a.seed)
    vcf = os.path.join(d, "cohort.vcf")
    subprocess.check_call([SAM_EXE, "-O", "v", "-a", "AD,DP", "--tile", str(a.tile), "-o", vcf, "-f", REF, "-r", "17:1-%d" % columns] + files)
    for f in files:
        os.remove(f)
    base = [CALL_EXE, "-v", "--timing", vcf]
    with_opt = base[:1] + ["--device-parse"] + base[1:]
    runs = {"host": [], "device": []}
    run(base), run(with_opt)                                                       # warm-up: the page cache, the code objects
    for _ in range(max(5, a.repeats)):                                             # alternating, in one visit
        runs["host"].append(run(base))
        runs["device"].append(run(with_opt))
    shas = {r["sha"] for rs in runs.values() for r in rs}
    lines.append("Cohort: %d single-sample SAM files, %.0fx, reads of %d bases over 17:1-%d of a random reference (seed %d): %d reads," %
                 (n_smpl, a.depth, RLEN, columns, a.seed, n_reads))
    lines.append("as VCF text of bcfgpu_sam -a AD,DP -O v: %d bytes.  bcfgpu_call -v: %d bytes of VCF text to a pipe; %d records' planes parsed on the device." %
                 (os.path.getsize(vcf), runs["host"][0]["nbytes"], runs["device"][0]["n_dev"]))
    lines.append("One warm-up run of each, then %d runs of each, alternating; seconds as --timing prints them, and the process's wall time." % len(runs["host"]))
    lines.append("")
    for kind in ("host", "device"):
        lines.append("%s path (%s):" % (kind, "the parent commit's text route: no option" if kind == "host" else "--device-parse"))
        for r in runs[kind]:
            lines.append("    %s    [wall %.3f]" % (r["line"], r["wall"]))
    lines.append("")
    lines.append("%-40s %26s %26s %12s" % ("seconds", "text route: median (spread)", "device: median (spread)", "difference"))
    verdicts = []
    for k in REPORTED:
        v = {kind: [r["vals"][k] for r in runs[kind]] for kind in runs}
        row = ["%.3f (%.3f)" % (statistics.median(v[kind]), max(v[kind]) - min(v[kind])) for kind in ("host", "device")]
        lines.append("%-40s %26s %26s %+12.3f" % (k, row[0], row[1], statistics.median(v["device"]) - statistics.median(v["host"])))
        verdicts.append(verdict(k, v["host"], v["device"]))
    lines.append("")
    lines.extend(verdicts)
    lines.append("")
    lines.append("outputs byte-equal in every run: %s (sha256 %s)" % ("yes" if len(shas) == 1 else "NO", sorted(shas)[0][:16]))
    lines.append("")
    os.remove(vcf)
    if len(shas) != 1:
        return "the outputs with and without --device-parse differ"
    if runs["device"][0]["n_dev"] <= 0 or any(r["n_dev"] for r in runs["host"]):
        return "--device-parse parsed no record on the device (or the plain run did)"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x16384,1000x4096", help="SAMPLESxCOLUMNS,...")
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5, help="runs of each path (at least 5)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_parse.txt"))
    ap.add_argument("--keep", metavar="DIR", help="work here instead of a temporary directory")
    a = ap.parse_args()
    tmp = None if a.keep else tempfile.TemporaryDirectory(prefix="bcfgpu_cohort_")
    d = a.keep or tmp.name
    os.makedirs(d, exist_ok=True)
    lines = ["bcfgpu_call -v --timing on VCF text, without and with --device-parse: tools/device_parse_timing.py, one MI355X, one GPU visit",
             "=" * 118, ""]
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
