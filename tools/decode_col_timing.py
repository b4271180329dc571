"""bcfgpu_call_decode_bcf with a sample map (`col`) on runs of more than one LDS slice: a pass over the called samples per
slice (the product) against lanes that read their sample from global memory (bcfdec.hip built with -DBCFDEC_COL_GLOBAL=1).

    python tools/decode_col_timing.py [--so OTHER_BUILD.so] [--records 400] [--samples 3000] [--repeats 20]

Times the entry itself (it synchronises the context's stream) on bytes already in HBM: int32 and int8 vectors of width 15,
col = NULL, the reversed samples and a random permutation; median and spread (largest - smallest) of --repeats calls after
two warm-up calls, per library, each library in a process of its own (BCFGPU_SO), the two alternating.  The planes of every
variant are compared with each other.  Not part of bench.py; fails without a GPU."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    from bcftools_amd import abi, engine
    from bcftools_amd.lib import check
    rng = np.random.default_rng(1)
    n, S, w = a.records, a.samples, 15
    res = {}
    with engine.Context(abi.default_cfg(S, max_sites=n, max_reads=64)) as ctx:
        out = ctx.buf(n * w * S * 4)
        for ty, dt in ((3, "<i4"), (1, "<i1")):
            per = S * w * np.dtype(dt).itemsize
            raw = rng.integers(0, 100, n * (per + 3) + 16, dtype=np.uint8)                     # runs 3 bytes apart from packed: every alignment
            d_in = ctx.to_device(raw)
            v = np.zeros(n, dtype=abi.BCF_VEC)
            v["off"], v["type"], v["width"] = np.arange(n) * (per + 3), ty, w
            for name, col in (("none", None), ("reversed", np.arange(S - 1, -1, -1, dtype=np.int32)), ("random", rng.permutation(S).astype(np.int32))):
                cp = None if col is None else col.ctypes.data_as(C.POINTER(C.c_int32))
                ts = []
                for i in range(a.repeats + 2):
                    t0 = time.perf_counter()
                    check(ctx.L.bcfgpu_call_decode_bcf(ctx.h, n, S, d_in.ptr, raw.nbytes, v.ctypes.data_as(C.POINTER(abi.BcfVec)), cp, w, out.ptr))
                    ts.append(time.perf_counter() - t0)
                got = out.download(np.zeros(n * w * S, np.int32))
                res["%s col=%s" % (dt, name)] = dict(ms=[1e3 * t for t in ts[2:]], sha=hashlib.sha256(got.tobytes()).hexdigest()[:16])
            ctx.release([d_in])
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--so", help="another build of the library to compare with the product")
    ap.add_argument("--records", type=int, default=400)
    ap.add_argument("--samples", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    libs = [("product (a pass per slice)", None)] + ([("other build (%s)" % os.path.basename(a.so), os.path.abspath(a.so))] if a.so else [])
    runs = {name: [] for name, _ in libs}
    for _ in range(2):                                                                         # alternating
        for name, so in libs:
            env = dict(os.environ)
            if so:
                env["BCFGPU_SO"] = so
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--records", str(a.records), "--samples", str(a.samples),
                                "--repeats", str(a.repeats)], env=env, check=True, stdout=subprocess.PIPE)
            runs[name].append(json.loads(p.stdout.decode().splitlines()[-1]))
    print("bcfgpu_call_decode_bcf, %d records x %d samples x width 15, n_planes 15; ms a call: median (spread) over 2 x %d calls" % (a.records, a.samples, a.repeats))
    shas = {}
    for case in runs[libs[0][0]][0]:
        row = []
        for name, _ in libs:
            ms = [x for r in runs[name] for x in r[case]["ms"]]
            row.append("%s: %.3f (%.3f)" % (name, statistics.median(ms), max(ms) - min(ms)))
            shas.setdefault(case, set()).update(r[case]["sha"] for r in runs[name])
        print("  %-22s %s" % (case, "    ".join(row)))
    print("planes equal across builds and runs: %s" % ("yes" if all(len(s) == 1 for s in shas.values()) else "NO"))


if __name__ == "__main__":
    main()
