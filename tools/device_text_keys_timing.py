"""What `bcfgpu_call --device-keys` does to the writer on VCF text input at cohort scale: the integer pass-through keys (AD, ADF, ADR,
DP, SP) of the records that are written made as BCF2 key blocks on the device from the input's own text
(bcfgpu_call_parse_keys_vcf), against the route `--device-parse --device-records -O u` leaves on the host for them (the record's
columns copied and split at tabs, every column at ':', every Number=R token at ',', all of it printed again, then split and parsed
a second time and typed, on one host thread).

    python tools/device_text_keys_timing.py [--samples 256] [--columns 16384] [--depth 30] [--tile 4096] [--repeats 3]
                                            [--out profiles/device_text_keys.txt] [--keep DIR]

The cohort is that of tools/device_records_timing.py, written as VCF text by `bcfgpu_sam -a AD,ADF,ADR,DP,SP -O v`.  `bcfgpu_call -m
-O u --device-parse --device-records --timing` (every record written) reads that file without and with --device-keys, alternating,
--repeats times each after one warm-up run of each.  The baseline is the run without the option: the parent commit's route.  Every
--timing line, the medians and the min-max spreads of "writing records", "uploads and device stages", their sum and the process's
wall time go to --out, then the kernels' times from one more run of the option's form under `rocprofv3 --kernel-trace --stats` (left
out, and said so, where rocprofv3 is not to be had).  No target is fixed; a gain (or a loss) is claimed only where the medians differ
by more than both spreads.  The outputs must be byte-equal in every run; the tool fails if they are not, and it fails without a GPU."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_call_rewrite_timing as rw  # noqa: E402
from device_parse_timing import CALL_EXE, run  # noqa: E402
from device_records_timing import RLEN, ROOT, SAM_EXE, write_cohort  # noqa: E402

TAGS = "AD,ADF,ADR,DP,SP"
BASE = ["--device-parse", "--device-records"]
BOTH = "writing records + device stages"
REPORTED = ("writing records", "uploads and device stages", BOTH, "reading records", "wall time of the process")
KERNELS = ("keytxt_size_kernel", "keytxt_write_kernel", "vcfdec_index_kernel", "vcfdec_parse_kernel")


def key_counts(cmd):
    """(N, M) of the option's --timing line."""
    err = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, check=True).stderr.decode()
    m = re.search(r"device keys: (\d+) pass-through key blocks made on the device, (\d+) on the host", err)
    return (int(m.group(1)), int(m.group(2))) if m else (0, 0)


def verdict(name, base, opt):
    mb, mo = statistics.median(base), statistics.median(opt)
    if abs(mo - mb) > max(max(base) - min(base), max(opt) - min(opt)):
        return "%s: %s with --device-keys (%.3f -> %.3f s, the difference exceeds both spreads)" % (name, "less" if mo < mb else "MORE", mb, mo)
    return "%s: no difference claimed (%.3f vs %.3f s, within the spreads %.3f-%.3f and %.3f-%.3f)" % (name, mb, mo, min(base), max(base), min(opt), max(opt))


def compare(a, d, vcf, lines):
    """The case in its two forms, alternating; appends its part of the report; a sentence when something is wrong."""
    base = [CALL_EXE, "-m", "-O", "u"] + BASE + ["--timing", vcf]
    with_opt = base[:1] + ["--device-keys"] + base[1:]
    n_dev, n_host = key_counts(with_opt)                                           # (also the warm-up of that form)
    run(base)
    runs = {"base": [], "keys": []}
    for _ in range(max(3, a.repeats)):                                             # alternating, in one visit
        runs["base"].append(run(base))
        runs["keys"].append(run(with_opt))
    for rs in runs.values():
        for r in rs:
            r["vals"][BOTH] = r["vals"]["writing records"] + r["vals"]["uploads and device stages"]
    shas = {r["sha"] for rs in runs.values() for r in rs}
    title = "bcfgpu_call -m -O u (every record is written)"
    lines.extend([title, "-" * len(title)])
    lines.append("Output: %d bytes of uncompressed BCF to a pipe; with --device-keys %d pass-through key blocks made on the device, %d on the host." %
                 (runs["base"][0]["nbytes"], n_dev, n_host))
    lines.append("One warm-up run of each form, then %d runs of each, alternating; seconds as --timing prints them, and the process's wall time." % len(runs["base"]))
    for kind, what in (("base", "%s: the parent commit's route, the baseline" % " ".join(BASE)), ("keys", "%s --device-keys" % " ".join(BASE))):
        lines.append("%s:" % what)
        for r in runs[kind]:
            lines.append("    %s    [wall %.3f]" % (r["line"], r["wall"]))
    lines.append("")
    lines.append("%-40s %32s %32s %12s" % ("seconds", "baseline: median (min - max)", "option: median (min - max)", "difference"))
    verdicts = []
    for k in REPORTED:
        v = {kind: [r["vals"][k] for r in runs[kind]] for kind in runs}
        row = ["%.3f (%.3f - %.3f)" % (statistics.median(v[kind]), min(v[kind]), max(v[kind])) for kind in ("base", "keys")]
        lines.append("%-40s %32s %32s %+12.3f" % (k, row[0], row[1], statistics.median(v["keys"]) - statistics.median(v["base"])))
        verdicts.append(verdict(k, v["base"], v["keys"]))
    lines.append("")
    lines.extend(verdicts)
    lines.append("")
    rw.KERNELS = KERNELS
    kt = rw.kernel_times([c for c in with_opt if c != "--timing"], d)
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
        return "the outputs with and without --device-keys differ"
    if n_dev <= 0 or n_host:
        return "--device-keys made no key block on the device (or left some to the host)"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--columns", type=int, default=16384)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3, help="runs of each form (at least 3)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_text_keys.txt"))
    ap.add_argument("--keep", metavar="DIR", help="work here instead of a temporary directory")
    a = ap.parse_args()
    tmp = None if a.keep else tempfile.TemporaryDirectory(prefix="bcfgpu_cohort_")
    d = a.keep or tmp.name
    os.makedirs(d, exist_ok=True)
    ref = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(a.seed).integers(0, 4, a.columns + RLEN)].tobytes().decode()
    REF = os.path.join(d, "ref.fa")
    with open(REF, "w") as f:
        f.write(">17\n" + "\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + "\n")
    files, n_reads = write_cohort(d, ref, a.samples, a.depth, a.columns, a.seed)
    vcf = os.path.join(d, "cohort.vcf")
    subprocess.check_call([SAM_EXE, "-O", "v", "-a", TAGS, "--tile", str(a.tile), "-o", vcf, "-f", REF, "-r", "17:1-%d" % a.columns] + files)
    for f in files:
        os.remove(f)
    lines = ["bcfgpu_call -m -O u --device-parse --device-records --timing on VCF text, without and with --device-keys: tools/device_text_keys_timing.py, one MI355X, one GPU visit",
             "=" * 150, ""]
    lines.append("Cohort: %d single-sample SAM files, %.0fx, reads of %d bases over 17:1-%d of a random reference (seed %d): %d reads," %
                 (a.samples, a.depth, RLEN, a.columns, a.seed, n_reads))
    lines.append("as VCF text of bcfgpu_sam -a %s -O v: %d bytes." % (TAGS, os.path.getsize(vcf)))
    lines.append("")
    bad = compare(a, d, vcf, lines)
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    if tmp:
        tmp.cleanup()
    if bad:
        raise SystemExit(bad)


if __name__ == "__main__":
    main()
