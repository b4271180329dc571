"""How much of a region's PCIe upload the staged read pool hides (bcfgpu_pool_stage / bcfgpu_pool_adopt).

    python tools/front_overlap.py [--regions 4] [--repeats 5] [--sites 16384] [--samples 1000] [--depth 30]
    python tools/front_overlap.py --serial-only            existing entry points only: runs on a tree without the staged pool
    python tools/front_overlap.py --pipelined-once         warm-up and one pipelined loop, for a timeline:
        rocprofv3 --kernel-trace --memory-copy-trace -f csv -d DIR -- python tools/front_overlap.py --pipelined-once
    python tools/front_overlap.py --timeline DIR           the relevant lines of that trace

The region of `bench.py --mode wgs` (bcftools_amd.synth.wgs_reads) with a seed per region, each pool copied into page-locked
buffers (bcfgpu_host_alloc).  After a warm-up of every region, two loops alternate in one process, each over all regions and
ending in one synchronise:
  serial     per region what bench.py's main_wgs does in front() and step(): bcfgpu_pool_upload, bcfgpu_pool_baq (flag 3),
             bcfgpu_pool_pileup, bcfgpu_pipeline + bcfgpu_compact_calls_async, bcfgpu_gap_prep_tile, and the pipeline + compaction
             on the indel tile
  pipelined  bcfgpu_pool_stage of region i + 1, the same stages on region i, bcfgpu_pool_adopt (the regions as a ring: the first
             region's pool is staged and adopted before the clock starts, and the last iteration stages the first region again,
             so both loops move every region's pool over PCIe once)
It prints one JSON line: ms per region of both loops (every repeat, the smallest, the spread = largest - smallest), the upload's
own time from page-locked and from pageable arrays, the share of it the pipelined loop got back, and whether the compacted
records of every region are byte-equal between the loops.  It fails without a GPU."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.append(ROOT)           # (behind PYTHONPATH: the serial leg is also run against another tree's bcftools_amd)


def timeline(d):
    """The host-to-device copies of at least 64 MiB (a region's bases and qualities) of the trace's last loop, and the kernels
    that ran inside the span of each."""
    def rows(pat):
        out = []
        for p in glob.glob(os.path.join(d, "**", pat), recursive=True):
            out += list(csv.DictReader(open(p)))
        return out
    kern, cop = rows("*kernel_trace.csv"), rows("*memory_copy_trace.csv")
    if not kern or not cop:
        raise SystemExit("no kernel_trace.csv / memory_copy_trace.csv under %s" % d)
    size_key = next((k for k in cop[0] if k.lower() in ("bytes", "size", "size_bytes")), None)
    h2d = [r for r in cop if "HOST_TO_DEVICE" in r.get("Direction", "").upper() or "H2D" in r.get("Direction", "").upper()]
    if size_key:
        big = [r for r in h2d if int(r[size_key]) >= (64 << 20)]
    else:                                                          # no size column: the long ones
        big = [r for r in h2d if int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) > 2000000]
    big.sort(key=lambda r: int(r["Start_Timestamp"]))
    ks = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in kern))
    t0 = int(big[0]["Start_Timestamp"]) if big else 0
    print("host-to-device copies of >= 64 MiB: %d in the trace (copy columns: %s)" % (len(big), ", ".join(cop[0].keys())))
    for r in big[-8:]:
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        inside = {}
        for a, b, name in ks:
            ov = min(e, b) - max(s, a)
            if ov > 0:
                name = name.replace("bcfgpu::", "").replace("void ", "").split("(")[0].split("<")[0]
                inside[name] = inside.get(name, 0) + ov
        tot = sum(inside.values())
        top = sorted(inside.items(), key=lambda kv: -kv[1])[:5]
        print("copy %s start %10.3f ms  dur %7.3f ms%s  kernels running inside its span: %7.3f ms  %s" %
              (r.get("Direction", "?"), (s - t0) / 1e6, (e - s) / 1e6, ("  %d MiB" % (int(r[size_key]) >> 20)) if size_key else "", tot / 1e6,
               ", ".join("%s %.2f" % (n, v / 1e6) for n, v in top)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sites", type=int, default=16384)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--serial-only", action="store_true")
    ap.add_argument("--pipelined-once", action="store_true")
    ap.add_argument("--timeline", metavar="DIR")
    a = ap.parse_args()
    if a.timeline:
        return timeline(a.timeline)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/front_overlap.py needs a GPU: the library has no CPU path")
    from bcftools_amd import abi, engine, synth
    from bcftools_amd.lib import check, load
    from tests.helpers import indeldrv
    Lib = load()
    S, n_sites, R = a.samples, a.sites, max(2, a.regions)
    pinned = []

    def pin(v):
        p = C.c_void_p()
        check(Lib.bcfgpu_host_alloc(max(v.nbytes, 1), C.byref(p)))
        pinned.append(p)
        w = np.ctypeslib.as_array((C.c_uint8 * max(v.nbytes, 1)).from_address(p.value))[:v.nbytes].view(v.dtype)
        w[...] = v
        return w

    # ---- the regions: page-locked pools; the first one also as the pageable arrays bench.py uploads from ----
    regs, pageable = [], None
    ctx0 = engine.Context(abi.default_cfg(S, max_sites=1, max_reads=64))
    for i in range(R):
        W = synth.wgs_reads(a.seed + i, n_sites, S, a.depth)
        arrs, mapq = W["reads"], W["mapq"]
        rd0 = abi.Reads()
        rd0.n_reads = W["n_reads"]
        for k, v in arrs.items():
            setattr(rd0, k, v.ctypes.data)
        ref_b = W["refseq"].encode()
        t = abi.Tile()
        check(ctx0.L.bcfgpu_pileup(ctx0.h, C.byref(rd0), mapq.ctypes.data, W["smpl"].ctypes.data, W["beg"], W["end"], ref_b, len(ref_b), C.byref(t), None, None))
        if i == 0:
            pageable = (rd0, arrs, mapq)
        keep = {k: pin(v) for k, v in arrs.items()}
        rd = abi.Reads()
        rd.n_reads = W["n_reads"]
        for k, v in keep.items():
            setattr(rd, k, v.ctypes.data)
        regs.append(dict(rd=rd, keep=keep, mapq=pin(mapq), smpl=W["smpl"], ref=ref_b, beg=W["beg"], end=W["end"], n=W["n_reads"],
                         entries=int(t.n_reads), bytes=sum(v.nbytes for v in arrs.values()) + mapq.nbytes,
                         col_n=np.zeros(n_sites, np.int32), col_indel=np.zeros(n_sites, np.uint8), tile=abi.Tile(), itile=abi.Tile()))
        if i:
            del W, arrs
    ctx0.close()
    ctx = engine.Context(abi.default_cfg(S, max_sites=n_sites, max_reads=max(r["entries"] for r in regs) + 64))
    Lb = ctx.L
    mo, mbufs, _ = ctx.alloc_mplp_out(n_sites, ctx.flagged_planes())
    co, cbufs, _ = ctx.alloc_call_out(n_sites, abi.MAX_PL)
    REC, IREC = 256 << 20, 64 << 20
    par_keep = []
    for r in regs:
        r["rec"], r["irec"] = torch.empty(REC, dtype=torch.uint8, device="cuda"), torch.empty(IREC, dtype=torch.uint8, device="cuda")
        r["cnt"], r["icnt"] = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
        par = abi.IndelIn()
        par.ref = r["ref"]
        for k, v in indeldrv.DEFAULTS.items():
            setattr(par, k, v)
        r["par"] = par
    CAP = indeldrv.CAP

    def upload(r):
        check(Lb.bcfgpu_pool_upload(ctx.h, C.byref(r["rd"]), None, r["mapq"].ctypes.data))

    def front(r):
        check(Lb.bcfgpu_pool_baq(ctx.h, r["ref"], len(r["ref"]), 3, None))
        check(Lb.bcfgpu_pool_pileup(ctx.h, r["smpl"].ctypes.data, None, r["beg"], r["end"], r["ref"], len(r["ref"]), C.byref(r["tile"]),
                                    r["col_n"].ctypes.data, r["col_indel"].ctypes.data))

    # warm-up, first half: every region's front, for its candidate columns (mpileup.c:354, -L 250) and the indel tile's size
    n_acc = 1
    for r in regs:
        upload(r)
        front(r)
        r["cand"] = np.ascontiguousarray(np.nonzero((r["col_indel"] != 0) & (r["col_n"] < 250 * S))[0], dtype=np.int32)
        nc = max(len(r["cand"]), 1)
        g = dict(ret=np.zeros(nc, np.int32), indel_types=np.zeros((nc, 4), np.int32), inscns=np.zeros((nc, 4 * CAP), np.int8), maxins=np.zeros(nc, np.int32),
                 indelreg=np.zeros(nc, np.int32), max_support=np.zeros(nc, np.int32), max_frac=np.zeros(nc, np.float32))
        oo = abi.IndelOut()
        oo.ret, oo.indel_types, oo.inscns = g["ret"].ctypes.data, g["indel_types"].ctypes.data, g["inscns"].ctypes.data
        oo.maxins, oo.indelreg, oo.max_support, oo.max_frac = g["maxins"].ctypes.data, g["indelreg"].ctypes.data, g["max_support"].ctypes.data, g["max_frac"].ctypes.data
        r["g"], r["oo"] = g, oo
        if len(r["cand"]):
            check(Lb.bcfgpu_gap_prep_tile(ctx.h, len(r["cand"]), r["cand"].ctypes.data, None, C.byref(r["par"]), C.byref(oo), CAP, C.byref(r["itile"])))
            n_acc = max(n_acc, int(r["itile"].n_sites))
    imo, imb, _ = ctx.alloc_mplp_out(n_acc, ctx.flagged_planes())
    ico, icb, _ = ctx.alloc_call_out(n_acc, abi.MAX_PL)

    def rest(r):
        check(Lb.bcfgpu_pipeline(ctx.h, C.byref(r["tile"]), None, None, C.byref(mo), C.byref(co)))
        check(Lb.bcfgpu_compact_calls_async(ctx.h, n_sites, 0, mo.site, C.byref(co), abi.MAX_PL, 2, r["rec"].data_ptr(), REC, r["cnt"].data_ptr()))
        if len(r["cand"]):
            check(Lb.bcfgpu_gap_prep_tile(ctx.h, len(r["cand"]), r["cand"].ctypes.data, None, C.byref(r["par"]), C.byref(r["oo"]), CAP, C.byref(r["itile"])))
            if r["itile"].n_sites:
                assert r["itile"].n_sites <= n_acc
                check(Lb.bcfgpu_pipeline(ctx.h, C.byref(r["itile"]), None, None, C.byref(imo), C.byref(ico)))
                check(Lb.bcfgpu_compact_calls_async(ctx.h, r["itile"].n_sites, 0, imo.site, C.byref(ico), abi.MAX_PL, 2, r["irec"].data_ptr(), IREC, r["icnt"].data_ptr()))

    def serial():
        t0 = time.perf_counter()
        for r in regs:
            upload(r)
            front(r)
            rest(r)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / R

    def pipelined():
        check(Lb.bcfgpu_pool_stage(ctx.h, C.byref(regs[0]["rd"]), None, regs[0]["mapq"].ctypes.data))
        check(Lb.bcfgpu_pool_adopt(ctx.h))
        ctx.sync()
        t0 = time.perf_counter()
        for i, r in enumerate(regs):
            nx = regs[(i + 1) % R]
            check(Lb.bcfgpu_pool_stage(ctx.h, C.byref(nx["rd"]), None, nx["mapq"].ctypes.data))
            front(r)
            rest(r)
            check(Lb.bcfgpu_pool_adopt(ctx.h))
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / R

    def records():
        out = []
        for r in regs:
            for buf, cnt, has in ((r["rec"], r["cnt"], True), (r["irec"], r["icnt"], bool(len(r["cand"]) and r["itile"].n_sites))):
                nb, nr = C.c_uint64(), C.c_uint32()
                if has:
                    check(Lb.bcfgpu_compact_counts(ctx.h, cnt.data_ptr(), C.byref(nb), C.byref(nr)))
                out.append((int(nr.value), buf[:int(nb.value)].cpu().numpy().tobytes()))
        return out
    have_stage = hasattr(Lb, "bcfgpu_pool_stage") and not a.serial_only
    # warm-up, second half: both loops once (every shape of every region, both sets of the pool's slots)
    serial()
    want = records()
    if have_stage:
        pipelined()
    if a.pipelined_once:
        ms = pipelined()
        print(json.dumps({"pipelined_ms_per_region": ms, "regions": R}), flush=True)
        return
    ser, pip, same = [], [], True
    for _ in range(max(1, a.repeats)):
        ser.append(serial())
        got = records()
        same = same and got == want
        if have_stage:
            pip.append(pipelined())
            same = same and records() == want
    # the upload alone (the call ends in a synchronise): page-locked, and from the pageable arrays of region 0

    def up_ms(rd, mapq):
        ts = []
        for _ in range(3):
            ctx.sync()
            t0 = time.perf_counter()
            check(Lb.bcfgpu_pool_upload(ctx.h, C.byref(rd), None, mapq.ctypes.data))
            ts.append((time.perf_counter() - t0) * 1e3)
        return min(ts)
    up_pin, up_page = up_ms(regs[0]["rd"], regs[0]["mapq"]), up_ms(pageable[0], pageable[2])
    out = {"regions": R, "columns": n_sites, "samples": S, "depth": a.depth, "reads_per_region": int(regs[0]["n"]), "pool_bytes_per_region": int(regs[0]["bytes"]),
           "records_per_region": [n for n, _ in want],
           "serial_ms_per_region": {"repeats": ser, "min": min(ser), "spread": max(ser) - min(ser)},
           "upload_ms": {"page_locked": up_pin, "pageable": up_page},
           "records_byte_equal_in_every_loop": bool(same)}
    if have_stage:
        out["pipelined_ms_per_region"] = {"repeats": pip, "min": min(pip), "spread": max(pip) - min(pip)}
        out["gain_ms_per_region"] = min(ser) - min(pip)
        out["recovered_share_of_upload"] = (min(ser) - min(pip)) / up_pin
        out["us_per_column"] = {"serial": min(ser) * 1e3 / n_sites, "pipelined": min(pip) * 1e3 / n_sites, "upload": up_pin * 1e3 / n_sites}
    print(json.dumps(out), flush=True)
    if not same:
        raise SystemExit("the compacted records differ between the loops")
    ctx.close()
    for p in pinned:
        check(Lib.bcfgpu_host_free(p))


if __name__ == "__main__":
    main()
