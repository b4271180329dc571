"""What `bcfgpu_call --device-alleles` does to a `-C alleles -T targets` run at cohort scale: the host rewrites the first nine columns
alone, the decoders make the input-shape planes on the device and bcfgpu_call_constrain gathers them into the planes mcall() reads --
against the host route (constrain_line() splits and prints every sample column of every changed record, build_planes() splits and
parses them again, the int32 planes cross PCIe).

    python tools/device_alleles_timing.py [--shapes 256x16384,1000x4096] [--depth 30] [--tile 4096] [--repeats 5]
                                          [--out profiles/device_alleles.txt] [--keep DIR]

Per shape (samples x columns) the cohort is that of tools/device_records_timing.py (its writer is imported), written as VCF text by
`bcfgpu_sam -a AD,DP -O v` and turned into BCF by bcfgpu_view; the targets file names every record and changes every second one: an
allele the record lacks where it has an unseen allele (<*>) to stand in for it, its last ALT dropped where all four bases were seen.
`bcfgpu_call -mA -C alleles -T targets --timing` runs without options (text in), with --device-parse --device-alleles (text in) and
with --device-input --device-alleles (BCF in), alternating, --repeats times each after one warm-up run of each; every --timing line, the medians and the spreads (largest - smallest) of "reading records", "building the planes on the
host", "uploads and device stages" and their sum go to --out.  The baseline is the same binary without the options -- the parent
commit's route -- in the same visit, and no ratio is expected in advance: a verdict line claims a difference only where the medians
differ by more than both spreads.  The outputs must be byte-equal in every run; the tool fails if they are not, and it fails without
a GPU (the drivers have no CPU path).  With --keep the last shape's inputs stay in DIR (for a kernel trace of one run)."""
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
VIEW_EXE = os.path.join(ROOT, "host", "bcfgpu_view")
FIELDS = ("reading records", "building the planes on the host", "uploads and device stages", "writing records")
SUM = "reading + host planes + device stages"
REPORTED = ("reading records", "building the planes on the host", "uploads and device stages", SUM, "wall time of the process")
ROUTES = (("host", "the parent commit's route: no option, text in"), ("parse", "--device-parse --device-alleles, text in"),
          ("input", "--device-input --device-alleles, BCF in"))


def run(cmd):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    if p.returncode:
        raise SystemExit("%s failed (%d):\n%s" % (" ".join(cmd[:8]), p.returncode, p.stderr.decode()[-2000:]))
    err = p.stderr.decode()
    line = next(ln for ln in err.splitlines() if "seconds: reading records" in ln)
    vals = {k: float(re.search(re.escape(k) + r" ([0-9.]+)", line).group(1)) for k in FIELDS}
    vals[SUM] = vals["reading records"] + vals["building the planes on the host"] + vals["uploads and device stages"]
    vals["wall time of the process"] = wall
    m = re.search(r"device alleles: (\d+) records' planes constrained on the device, (\d+) taken as they were", err)
    return dict(line=line, wall=wall, vals=vals, n_dev=(int(m.group(1)), int(m.group(2))) if m else (0, 0),
                sha=hashlib.sha256(p.stdout).hexdigest(), nbytes=len(p.stdout))


def verdict(name, what, host, dev):
    """A difference is claimed only where the medians differ by more than both spreads."""
    mh, md = statistics.median(host), statistics.median(dev)
    sh, sd = max(host) - min(host), max(dev) - min(dev)
    if abs(md - mh) > max(sh, sd):
        return "%s, %s: %s than the host route (%.3f -> %.3f s, the difference exceeds both spreads)" % (name, what, "less" if md < mh else "MORE", mh, md)
    return "%s, %s: no difference claimed (%.3f vs %.3f s, within the spreads %.3f and %.3f)" % (name, what, mh, md, sh, sd)


def write_targets(vcf, path):
    """A target for every record: its alleles (the unseen allele aside); every second one is changed -- with a base the record lacks
    where the record has an unseen allele to stand in for it, without its last ALT otherwise."""
    n = n_new = n_cut = 0
    with open(vcf) as f, open(path, "w") as o:
        for ln in f:
            if ln.startswith("#"):
                continue
            c = ln.split("\t", 5)
            real = [a for a in c[4].split(",") if a != "." and not a.startswith("<")]
            als = [c[3]] + real
            if n % 2:
                # A new allele takes the unseen allele's values, so only a record that has one (<*>) can get it (without one the
                # site is skipped, mcall.c:1294-1303); a site where all four bases were seen has none, and loses its last ALT
                # instead: changed either way, the planes gathered into a narrower record
                lacks = [b for b in "ACGT" if b not in {c[3][0].upper()} | {a.upper() for a in real}]
                if lacks and len(real) < len(c[4].split(",")):
                    als = [c[3]] + real[:2] + [lacks[0] + c[3][1:]]
                    n_new += 1
                elif real:
                    als = [c[3]] + real[:-1]
                    n_cut += 1
            o.write("%s\t%s\t%s\n" % (c[0], c[1], ",".join(als)))
            n += 1
    return n, n_new, n_cut


def one_shape(a, d, n_smpl, columns, lines):
    ref = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(a.seed).integers(0, 4, columns + RLEN)].tobytes().decode()
    REF = os.path.join(d, "ref.fa")
    with open(REF, "w") as f:
        f.write(">17\n" + "\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + "\n")
    files, n_reads = write_cohort(d, ref, n_smpl, a.depth, columns, a.seed)
    vcf, bcf, tab = os.path.join(d, "cohort.vcf"), os.path.join(d, "cohort.bcf"), os.path.join(d, "targets.tab")
    subprocess.check_call([SAM_EXE, "-O", "v", "-a", "AD,DP", "--tile", str(a.tile), "-o", vcf, "-f", REF, "-r", "17:1-%d" % columns] + files)
    for f in files:
        os.remove(f)
    subprocess.check_call([VIEW_EXE, "-O", "u", "-o", bcf, vcf])
    n_tgt, n_new, n_cut = write_targets(vcf, tab)
    base = [CALL_EXE, "-m", "-A", "-C", "alleles", "-T", tab, "--timing"]
    cmds = {"host": base + [vcf], "parse": base + ["--device-parse", "--device-alleles", vcf], "input": base + ["--device-input", "--device-alleles", bcf]}
    runs = {k: [] for k in cmds}
    for k in cmds:                                                                 # warm-up: the page cache, the code objects
        run(cmds[k])
    for _ in range(max(5, a.repeats)):                                             # alternating, in one visit
        for k in cmds:
            runs[k].append(run(cmds[k]))
    shas = {r["sha"] for rs in runs.values() for r in rs}
    lines.append("Cohort: %d single-sample SAM files, %.0fx, reads of %d bases over 17:1-%d of a random reference (seed %d): %d reads," %
                 (n_smpl, a.depth, RLEN, columns, a.seed, n_reads))
    lines.append("as VCF text of bcfgpu_sam -a AD,DP -O v: %d bytes, as BCF (-O u): %d bytes; %d targets, %d of them with an allele the record lacks, %d without the record's last ALT." %
                 (os.path.getsize(vcf), os.path.getsize(bcf), n_tgt, n_new, n_cut))
    lines.append("bcfgpu_call -mA -C alleles -T: %d bytes of VCF text to a pipe; %d records' planes constrained on the device, %d taken as they were." %
                 ((runs["host"][0]["nbytes"],) + runs["parse"][0]["n_dev"]))
    lines.append("One warm-up run of each, then %d runs of each, alternating; seconds as --timing prints them, and the process's wall time." % len(runs["host"]))
    lines.append("")
    for kind, what in ROUTES:
        lines.append("%s:" % what)
        for r in runs[kind]:
            lines.append("    %s    [wall %.3f]" % (r["line"], r["wall"]))
    lines.append("")
    lines.append("%-40s %24s %24s %24s" % ("seconds: median (spread)", "host route", "--device-parse + alleles", "--device-input + alleles"))
    verdicts = []
    for k in REPORTED:
        v = {kind: [r["vals"][k] for r in runs[kind]] for kind in runs}
        row = ["%.3f (%.3f)" % (statistics.median(v[kind]), max(v[kind]) - min(v[kind])) for kind, _ in ROUTES]
        lines.append("%-40s %24s %24s %24s" % (k, row[0], row[1], row[2]))
        verdicts += [verdict(k, what, v["host"], v[kind]) for kind, what in ROUTES[1:]]
    lines.append("")
    lines.extend(verdicts)
    lines.append("")
    lines.append("outputs byte-equal in every run: %s (sha256 %s)" % ("yes" if len(shas) == 1 else "NO", sorted(shas)[0][:16]))
    lines.append("")
    if not a.keep:
        for p in (vcf, bcf, tab):
            os.remove(p)
    if len(shas) != 1:
        return "the outputs with and without the options differ"
    if any(r["n_dev"][0] <= 0 for k in ("parse", "input") for r in runs[k]) or any(sum(r["n_dev"]) for r in runs["host"]):
        return "--device-alleles constrained no record on the device (or the plain run did)"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x16384,1000x4096", help="SAMPLESxCOLUMNS,...")
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5, help="runs of each route (at least 5)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_alleles.txt"))
    ap.add_argument("--keep", metavar="DIR", help="work here instead of a temporary directory, and leave the last shape's inputs there")
    a = ap.parse_args()
    tmp = None if a.keep else tempfile.TemporaryDirectory(prefix="bcfgpu_cohort_")
    d = a.keep or tmp.name
    os.makedirs(d, exist_ok=True)
    lines = ["bcfgpu_call -mA -C alleles -T targets --timing, without options and with --device-alleles on text and on BCF input: "
             "tools/device_alleles_timing.py, one MI355X, one GPU visit", "=" * 118, ""]
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
