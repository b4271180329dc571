#!/usr/bin/env python3
"""Register and instruction counts of glfgen_kernel's phase-A loop, from the ISA a --save-temps build leaves (no GPU needed).

usage: python3 tools/glf_isa.py <glfgen-hip-amdgcn-amd-amdhsa-gfx950.s> [kernel name substring, default ILb0ELb1ELb0E]

Build the listing with the Makefile's options for glfgen.hip, e.g. in a scratch copy of csrc/:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off $(make -s print-flags-glfgen) --save-temps -c glfgen.hip

Phase A's loop is taken from LLVM's loop annotations in the listing ("; =>This Inner Loop Header", "in Loop: Header=BBx",
"Parent Loop BBx"): the innermost loop whose blocks (nested loops included) hold the byte-plane sums (v_dot4_u32_u8 /
v_dot2_u32_u16) and no double-precision instruction.  Printed per block of that loop, in listing order: the vector ALU
instructions (v_*, which is what SQ_INSTS_VALU counts), v_readlane / v_writelane among them, LDS and global/flat memory
instructions, and the block's IR name.  The totals count every block once (a static count: rare blocks such as the
tile-tail fetch or the diff-read sums are included); reads per trip: 4 per lane."""
import re
import sys


def functions(lines):
    cur, body = None, []
    for ln in lines:
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", ln)
        if m:
            if cur:
                yield cur, body
            cur, body = m.group(1), []
        elif cur:
            if re.match(r"^\s*\.Lfunc_end", ln):
                yield cur, body
                cur, body = None, []
            else:
                body.append(ln)


def meta(text, name):
    i = text.find(".name:           " + name)
    blk = text[i:i + 1500]
    get = lambda k: (re.search(r"\." + k + r":\s+(\d+)", blk) or [None, "?"])[1]
    return {k: get(k) for k in ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}


def blocks(body):
    """Basic blocks in listing order: label, IR name, innermost loop header (or None), parent loops of a header, instructions."""
    out, cur = [], None
    for ln in body:
        code, _, com = ln.partition(";")
        code = code.strip()
        m = re.match(r"^(\.LBB\S+):$", code) or (re.match(r"^%bb\.(\d+):", com.strip()) if not code else None)
        if m:
            lab = m.group(1) if code else "%bb." + m.group(1)
            cur = dict(lab=lab, name=com.strip() if code else "", hdr=None, parents=[], ins=[])
            out.append(cur)
        elif cur is None:
            cur = dict(lab="<entry>", name="", hdr=None, parents=[], ins=[])
            out.append(cur)
        if cur is not None:
            mh = re.search(r"in Loop: Header=(BB\S+)", com)
            if mh:
                cur["hdr"] = mh.group(1)
            if re.search(r"This (Inner )?Loop Header", com):
                cur["hdr"] = cur["lab"].lstrip(".L")
            mp = re.search(r"Parent Loop (BB\S+)", com)
            if mp:
                cur["parents"].append(mp.group(1))
            if code and not code.startswith(".") and not re.match(r"^\S+:$", code):
                cur["ins"].append(code)
    return out


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "ILb0ELb1ELb0E"
    text = open(path).read()
    for name, body in functions(text.splitlines()):
        if "glfgen_kernel" not in name or want not in name:
            continue
        md = meta(text, name)
        bl = blocks(body)
        allv = [i for b in bl for i in b["ins"] if i.startswith("v_")]
        print(name)
        print("  " + " ".join("%s=%s" % kv for kv in md.items()))
        print("  whole kernel: %d v_* instructions, %d v_readlane, %d v_writelane" % (
            len(allv), sum(i.startswith("v_readlane") for i in allv), sum(i.startswith("v_writelane") for i in allv)))
        # loop tree: header -> parent header
        parent = {}
        for b in bl:
            if b["hdr"] == b["lab"].lstrip(".L") and b["parents"]:
                parent[b["hdr"]] = b["parents"][-1]
        def within(h, loop):
            while h is not None:
                if h == loop:
                    return True
                h = parent.get(h)
            return False
        cand = []
        for loop in {b["hdr"] for b in bl if b["hdr"]}:
            mem = [b for b in bl if b["hdr"] and within(b["hdr"], loop)]
            ins = [i for b in mem for i in b["ins"]]
            if any(re.match(r"v_dot[24]", i) for i in ins) and not any(re.match(r"v_(fma|add|mul)_f64", i) for i in ins):
                cand.append((len(ins), loop, mem))
        if not cand:
            print("  phase-A loop not found")
            continue
        _, loop, mem = min(cand, key=lambda c: c[0])
        tot = dict(v=0, rl=0, wl=0, ds=0, gl=0)
        print("  phase-A loop: header %s, %d blocks" % (loop, len(mem)))
        for b in mem:
            ins = b["ins"]
            v = [i for i in ins if i.startswith("v_")]
            c = dict(v=len(v), rl=sum(i.startswith("v_readlane") for i in v), wl=sum(i.startswith("v_writelane") for i in v),
                     ds=sum(i.startswith("ds_") for i in ins), gl=sum(i.startswith(("global_", "buffer_", "flat_")) for i in ins))
            for key in tot:
                tot[key] += c[key]
            print("    %-10s v_*=%3d readlane=%2d writelane=%2d ds=%2d mem=%2d  %s" % (
                b["lab"], c["v"], c["rl"], c["wl"], c["ds"], c["gl"], b["name"][:60]))
        print("  loop total (static, every block once): v_*=%d readlane=%d writelane=%d ds=%d mem=%d" % (
            tot["v"], tot["rl"], tot["wl"], tot["ds"], tot["gl"]))


if __name__ == "__main__":
    main()
