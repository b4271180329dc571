#!/usr/bin/env python3
"""Register and instruction counts of glfgen_kernel's loops, from the ISA a --save-temps build leaves (no GPU needed).

usage: python3 tools/glf_isa.py <glfgen-hip-amdgcn-amd-amdhsa-gfx950.s> [kernel name substring, default ILb0ELb1ELb0E]

Build the listing with the Makefile's options for glfgen.hip, e.g. in a scratch copy of csrc/:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off $(make -s print-flags-glfgen) --save-temps -c glfgen.hip
(or --cuda-device-only -S -o <listing>).

Phase A's loops are taken from LLVM's loop annotations in the listing ("; =>This Inner Loop Header", "in Loop: Header=BBx",
"Parent Loop BBx"): the loops whose blocks (nested loops included) hold the byte-plane sums (v_dot4_u32_u8 /
v_dot2_u32_u16) and no double-precision instruction.  The smallest one that stores single keys (a ragged end of a segment) is
the general loop; the smallest one that does not is the full-trip loop, which lies inside it and is reported first, with its
trips a pass (a key store a trip) and the instructions a full trip must not need.  Printed per block of that loop, in listing order: the vector ALU
instructions (v_*, which is what SQ_INSTS_VALU counts), v_readlane / v_writelane among them, LDS and global/flat memory
instructions, and the block's IR name.  The totals count every block once (a static count: rare blocks such as the
tile-tail fetch or the diff-read sums are included); reads per trip: 4 per lane.

Phase B's loops follow, each found by what it holds, not by its label (static counts, every block of the loop once):
  pass 1      the innermost loop with the swap of a rare read (two ds_write_b16) and the 64-bit shift of the quality mask, no
              global load; keys a trip = its ds_read_u16 outside the swap blocks
  count_runs  every innermost loop with FU = 4 ds_add_u32 and ds_read_u16 and no byte-plane sum: "first" when it shifts the
              mask once a key (the rank), "later" when twice (the test of the quality as well); "rank test" when it compares
              with a constant after the population counts; the nesting depth tells the primary base (the shallower loops) from
              the other bases
  rank code   "the quality of every rank joins its counts": the blocks that read and write one slot dword (ds_read_b32 and
              ds_write_b32) with the v_ffbh_u32 blocks around them -- a loop, or the unrolled copies, then counted per copy
  walk        the innermost loops with four global_load_dwordx2 and double-precision arithmetic, with the s_waitcnt that
              opens the trip; and the walk's start, from the prefix-table load to the loop (walk_start below)

The straight-line code around the loops comes last (straight_line below): the prologue up to the rounds' loop, the 15
likelihoods of a cell with two or more bases, and the other bases' short paths."""
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
        # the general loop stores single keys at a ragged end (ds_write_b16; the DEEP forms keep their keys in global memory:
        # global_store_short); the full-trip loop inside it stores whole quads only, and its blocks are not counted again
        ragged = lambda c: any(i.startswith(("ds_write_b16", "global_store_short", "flat_store_short")) for b in c[2] for i in b["ins"])
        full = min([c for c in cand if not ragged(c)], key=lambda c: c[0], default=None)
        gen = min([c for c in cand if ragged(c)], key=lambda c: c[0], default=None)
        _, loop, mem = gen or full
        inner = {id(b) for b in full[2]} if full and gen else set()
        def report(tag, loop, mem, trips):
            tot = dict(v=0, rl=0, wl=0, ds=0, gl=0)
            print("  %s: header %s, %d blocks" % (tag, loop, len(mem)))
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
            return tot
        if full and gen:
            fmem = full[2]
            fins = [i for b in fmem for i in b["ins"]]
            # trips a pass: a trip stores its keys once (8 bytes a lane)
            trips = max(1, cnt(fins, "ds_write_b64", "global_store_dwordx2", "flat_store_dwordx2"))
            tot = report("phase-A full-trip loop", full[1], fmem, trips)
            movs = sum(bool(re.match(r"v_mov_b32\S*\s+v\d+, v\d+$", i)) for i in fins)
            print("  full trips a pass: %d, v_* a trip: %.1f; register copies (v_mov_b32 v, v)=%d flat_load=%d v_lshl_add_u64=%d ds_write_b16=%d" % (
                trips, tot["v"] / trips, movs, cnt(fins, "flat_load"), cnt(fins, "v_lshl_add_u64"), cnt(fins, "ds_write_b16")))
            report("phase-A general loop (without the full-trip loop's blocks)", loop, [b for b in mem if id(b) not in inner], 1)
        else:
            report("phase-A loop", loop, mem, 1)
        phase_b(bl, parent, {id(b) for b in mem})
        straight_line(bl, parent, loop)


def cnt(ins, *prefix):
    return sum(i.startswith(prefix) for i in ins)


def straight_line(bl, parent, phase_a_loop):
    """The code run once per workgroup or once per cell and round, by content (static counts, every block once):
      prologue         every block in front of the header of the rounds' loop (the outermost loop around phase A's)
      two-base cells   the 15 likelihoods of a cell with reads of two or more bases: from the first to the last block that widens a
                       float accumulator (v_cvt_f64_f32; the single-base store needs none), a loop over such cells when it reads
                       them with ds_bpermute_b32
      other bases      the loop over the five bases (the loop around the deepest count_runs loops) without its count_runs, rank
                       and walk blocks, i.e. its "no cell shows a base twice" path with the key loop; and the one-product form:
                       the block outside every inner loop with one v_mul_f64, one v_add_f64 and one 8-byte global load"""
    rounds = phase_a_loop
    while parent.get(rounds) is not None:
        rounds = parent[rounds]
    k0 = next(k for k, b in enumerate(bl) if b["lab"].lstrip(".L") == rounds)
    pro = [i for b in bl[:k0] for i in b["ins"]]
    print("  straight-line code:")
    print("  %-34s %d blocks: v_*=%3d of them v_rcp*=%d v_mad_u64_u32=%d; s_*=%d" % (
        "prologue, to the rounds' loop", k0, cnt(pro, "v_"), cnt(pro, "v_rcp"), cnt(pro, "v_mad_u64_u32"), cnt(pro, "s_")))
    wide = [k for k, b in enumerate(bl) if cnt(b["ins"], "v_cvt_f64_f32")]
    two = set()
    if wide:
        # a block inside a loop of its own brings the whole loop; behind the last one, the blocks that still narrow a sum
        inner = {bl[k]["hdr"] for k in wide if bl[k]["hdr"] != rounds}
        wide += [k for k, b in enumerate(bl) if b["hdr"] in inner]
        last = max(wide)
        while last + 1 < len(bl) and bl[last + 1]["hdr"] == bl[last]["hdr"] and last + 1 - max(wide) <= 3:
            last += 1
            if cnt(bl[last]["ins"], "v_cvt_f32_f64"):
                wide.append(last)
        mem = bl[min(wide):max(wide) + 1]
        two = {id(b) for b in mem}
        ins = [i for b in mem for i in b["ins"]]
        print("  %-34s from %-9s %2d blocks: v_*=%3d (f64 add/mul/cvt=%d) ds_bpermute=%d mem=%d%s" % (
            "two-base cells", mem[0]["lab"], len(mem), cnt(ins, "v_"), cnt(ins, "v_add_f64", "v_mul_f64", "v_cvt_f64", "v_cvt_f32_f64"),
            cnt(ins, "ds_bpermute"), cnt(ins, "global_", "buffer_", "flat_"), "  a loop, a trip a cell" if inner else "  once a wavefront"))
    def depth(h):
        d = 1
        while parent.get(h) is not None:
            h, d = parent[h], d + 1
        return d
    hdrs = {b["hdr"] for b in bl if b["hdr"]}
    def within(h, loop):
        while h is not None:
            if h == loop:
                return True
            h = parent.get(h)
        return False
    deepest = max((depth(h) for h in hdrs), default=0)
    counters = [h for h in hdrs if depth(h) == deepest and cnt([i for b in bl if b["hdr"] == h for i in b["ins"]], "ds_add_u32") == 4]
    if counters and deepest >= 3:
        base = counters[0]
        while depth(base) > 2:
            base = parent[base]
        # the blocks of the base loop itself and of its inner loops that neither count (ds_add_u32), rank (ds_write_b32) nor walk
        keep = []
        for h in hdrs:
            if within(h, base):
                ins = [i for b in bl if b["hdr"] and within(b["hdr"], h) for i in b["ins"]]
                if h == base or not (cnt(ins, "ds_add_u32") or cnt(ins, "ds_write_b32") or cnt(ins, "v_fma_f64", "v_mul_f64") > 1):
                    keep += [b for b in bl if b["hdr"] == h]
        ins = [i for b in keep for i in b["ins"]]
        print("  %-34s header %-9s %2d blocks: v_*=%3d ds=%2d mem=%2d (a trip a base present in the wavefront)" % (
            "other bases, the loop's short path", base, len(keep), cnt(ins, "v_"), cnt(ins, "ds_"), cnt(ins, "global_", "buffer_", "flat_")))
    for b in bl:
        ins = b["ins"]
        if b["hdr"] == rounds and cnt(ins, "v_mul_f64") == 1 and cnt(ins, "v_add_f64") == 1 and cnt(ins, "global_load_dwordx2") == 1 \
                and id(b) not in two:
            print("  %-34s block  %-9s           v_*=%3d ds=%2d mem=%2d" % (
                "other bases, one product a lane", b["lab"], cnt(ins, "v_"), cnt(ins, "ds_"), cnt(ins, "global_", "buffer_", "flat_")))


def phase_b(bl, parent, phase_a):
    """The loops of phase B, by content (see the module's docstring); `phase_a`: the blocks of phase A's loop."""
    def depth(h):
        d = 1
        while parent.get(h) is not None:
            h, d = parent[h], d + 1
        return d
    hdrs = [b["hdr"] for b in bl if b["hdr"] == b["lab"].lstrip(".L")]
    inner = [h for h in hdrs if h not in parent.values()]
    loops = {h: [b for b in bl if b["hdr"] == h] for h in inner}
    def line(tag, h, mem, extra=""):
        ins = [i for b in mem for i in b["ins"]]
        print("  %-34s header %-9s depth %d, %2d blocks: v_*=%3d ds=%2d mem=%2d%s" % (
            tag, h, depth(h), len(mem), cnt(ins, "v_"), cnt(ins, "ds_"), cnt(ins, "global_", "buffer_", "flat_"), extra))
    print("  phase B:")
    skip = set(phase_a)
    for h in inner:
        mem = loops[h]
        ins = [i for b in mem for i in b["ins"]]
        glob, dot = cnt(ins, "global_", "buffer_", "flat_"), sum(bool(re.match(r"v_dot[24]", i)) for i in ins)
        if cnt(ins, "ds_write_b16") >= 2 and cnt(ins, "v_lshlrev_b64") and not glob and not dot:
            keys = sum(cnt(b["ins"], "ds_read_u16") for b in mem if not cnt(b["ins"], "ds_write_b16"))
            # the common path: without the blocks of the rare read, from the one that swaps it (behind an s_cbranch_execz) round
            # the loop to that branch's target
            rare = set()
            for k, b in enumerate(mem):
                nxt = mem[(k + 1) % len(mem)]
                m = re.match(r"s_cbranch_execz\s+(\S+)", b["ins"][-1]) if b["ins"] else None
                if m and cnt(nxt["ins"], "ds_write_b16"):
                    j = (k + 1) % len(mem)
                    while mem[j]["lab"] != m.group(1) and len(rare) < len(mem):
                        rare.add(j)
                        j = (j + 1) % len(mem)
            common = [i for k, b in enumerate(mem) if k not in rare for i in b["ins"]]
            line("pass 1, %d keys a trip" % keys, h, mem, "  common path (no rare read): v_*=%d ds=%d" % (cnt(common, "v_"), cnt(common, "ds_")))
        elif cnt(ins, "ds_add_u32") == 4 and cnt(ins, "ds_read_") and not dot:
            skip.update(id(b) for b in mem)
            later = cnt(ins, "v_lshrrev_b64") > 4
            chk = any(re.match(r"v_cmpx?_(gt|lt|le|ge)_u(32|64)\S*\s+(vcc|s\[\d+:\d+\]), (10|9), ", i) or
                      re.match(r"v_cmpx?_(gt|lt|le|ge)_u(32|64)\S*\s+(10|9), ", i) for i in ins)
            line("count_runs<%s>, %s, 4 keys" % ("false" if later else "true", "rank test" if chk else "no rank test"), h, mem)
        elif glob >= 4 and any(re.match(r"v_(fma|add|mul)_f64", i) for i in ins):
            wait = next((i for i in mem[0]["ins"] if i.startswith("s_waitcnt")), "none in the header block")
            line("walk_runs trip", h, mem, "  opens with: " + wait)
            walk_start(bl, mem[0])
    # the rank code: slot dwords read and written back
    upd = [k for k, b in enumerate(bl) if cnt(b["ins"], "ds_read_b32") and cnt(b["ins"], "ds_write_b32") and id(b) not in skip]
    groups = []
    for k in upd:
        if groups and k - groups[-1][-1] <= 4:
            groups[-1].append(k)
        else:
            groups.append([k])
    done = set()
    for g in groups:
        h = bl[g[0]]["hdr"]
        if h in loops and any(cnt(b["ins"], "v_ffbh_u32") for b in loops[h]):
            if h not in done:
                line("rank code, a loop: a trip a rank", h, loops[h])
                done.add(h)
            continue
        # unrolled: a copy = the blocks from one that holds (or follows) the v_ffbh_u32 pair up to the next copy's; the last
        # copy runs into the code behind it and is left out of the figure
        first = lambda k: k - 1 if k and cnt(bl[k - 1]["ins"], "v_ffbh_u32") and not cnt(bl[k]["ins"], "v_ffbh_u32") else k
        if len(g) < 2 or not any(cnt(b["ins"], "v_ffbh_u32") for b in bl[first(g[0]):g[-1] + 1]):
            continue
        per = []
        for k0, k1 in zip(g, g[1:]):
            ins = [i for b in bl[first(k0):first(k1)] for i in b["ins"]]
            per.append((cnt(ins, "v_"), cnt(ins, "ds_")))
        per.sort()
        v, d = per[len(per) // 2]
        print("  %-34s from %-9s depth %d, %2d copies: v_*=%3d ds=%2d a rank (the median copy)" % (
            "rank code, unrolled", bl[first(g[0])]["lab"], depth(h) + 1 if h else 1, len(g), v, d))


def walk_start(bl, header):
    """The walk's start: from the prefix-table load (the last global_load_dwordx2 with a 64-bit vector address in front of the
    walk's loop; the walk's own loads address beta from a scalar base) to the loop's header -- the loads issued behind it and
    every s_waitcnt vmcnt on the way (vmcnt(0) right behind the load: the table entry is waited for on its own)."""
    k = next(i for i, b in enumerate(bl) if b is header)
    seq = [i for b in bl[:k] for i in b["ins"]]
    at = next((j for j in range(len(seq) - 1, -1, -1) if re.match(r"global_load_dwordx2\s+v\[\d+:\d+\], v\[\d+:\d+\], off", seq[j])), None)
    if at is None or len(seq) - at > 400:
        print("    walk start: no prefix-table load in front of the loop")
        return
    tail = seq[at + 1:]
    waits = ["%s after %d more loads" % (i.split(None, 1)[1], cnt(tail[:j], "global_load")) for j, i in enumerate(tail)
             if i.startswith("s_waitcnt") and "vmcnt" in i]
    print("    walk start: table load to loop header %d instructions, v_*=%d, loads behind it=%d; vmcnt waits: %s" % (
        len(tail), cnt(tail, "v_"), cnt(tail, "global_load"), "; ".join(waits) or "none"))


if __name__ == "__main__":
    main()
