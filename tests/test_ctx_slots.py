"""The context's workspace slot table (bcftools_amd/csrc/ctx.h) against the rules its comments state: a kept slot (WS_KEPT)
belongs to one entry point and shares its number with no other use; inside one call two names share a number only where this
file names the alias; every slot is below WS_COUNT / PINNED_COUNT.  CPU only: the enums are read from the header's text."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTX_H = os.path.join(ROOT, "bcftools_amd", "csrc", "ctx.h")

# the entry points and the name prefixes of the slots each takes during one call (a prefix may serve several calls)
CALLS = {
    "bcfgpu_baq": ("WS_VIEW_", "WS_BAQ_", "WS_PBAQ_"),              # the view of the caller's reads, its outputs, baq_core's scratch
    "bcfgpu_overlap_tweak": ("WS_VIEW_", "WS_POVL_"),
    "bcfgpu_cap_mapq": ("WS_VIEW_", "WS_PCAPQ_", "WS_POOL_EXTENT"),
    "bcfgpu_pool_upload": ("WS_POOL_",),
    "bcfgpu_pool_keep": ("WS_POOL_KEEP",),
    "bcfgpu_pool_baq": ("WS_PBAQ_",),
    "bcfgpu_pool_overlap_tweak": ("WS_POVL_",),
    "bcfgpu_pool_cap_mapq": ("WS_PCAPQ_", "WS_POOL_EXTENT"),
    "bcfgpu_pool_pileup": ("WS_PLP_",),
    "bcfgpu_pileup": ("WS_POOL_", "WS_PLP_"),
    "bcfgpu_pileup_entries": ("WS_ENT_",),
    "bcfgpu_pileup_indel_tile": ("WS_ITILE_",),
    "bcfgpu_gap_prep": ("WS_VIEW_", "WS_GAP_"),
    "bcfgpu_gap_prep_tile": ("WS_GTILE_", "WS_VIEW_", "WS_GAP_"),
    "bcfgpu_gvcf_blocks": ("WS_GVCF_",),
    "bcfgpu_compact_calls": ("WS_COMPACT_",),
    "bcfgpu_errmod_plan": ("WS_DRAW_",),
}
# the one buffer a call takes for two things, one after the other: (name, name) pairs, order free
ALIASES = {
    frozenset(("WS_PLP_SCAN_TMP", "WS_PLP_RECS")),       # the scan's temporary storage is done with before the records go there
}
# the entry point whose slot a kept name is: its prefix
OWNER_PREFIXES = sorted({p for ps in CALLS.values() for p in ps}, key=len, reverse=True)


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def parse_enum(text, name):
    """{enumerator: value} of `enum name : int { ... };` (values: integers, or another enumerator plus an integer)."""
    m = re.search(r"enum\s+%s\s*:\s*int\s*\{(.*?)\};" % name, _strip_comments(text), flags=re.S)
    assert m, "enum %s not found in ctx.h" % name
    vals = {}
    for item in m.group(1).split(","):
        item = item.strip()
        if not item:
            continue
        k, _, expr = (x.strip() for x in item.partition("="))
        assert expr, "%s has no explicit value" % k
        e = re.fullmatch(r"(\d+)|([A-Z_][A-Z0-9_]*)\s*\+\s*(\d+)", expr)
        assert e, "%s = %s: not a form this test reads" % (k, expr)
        vals[k] = int(e.group(1)) if e.group(1) else vals[e.group(2)] + int(e.group(3))
    return vals


def parse_kept(text):
    m = re.search(r"constexpr\s+WsSlot\s+WS_KEPT\s*\[\s*\]\s*=\s*\{(.*?)\};", _strip_comments(text), flags=re.S)
    assert m, "ctx.h declares no WS_KEPT list"
    return [x.strip() for x in m.group(1).split(",") if x.strip()]


def owner(name):
    for p in OWNER_PREFIXES:
        if name.startswith(p):
            return p
    return None


def slot_violations(text):
    """The rules above, as a list of messages (empty: the table keeps them)."""
    ws = parse_enum(text, "WsSlot")
    count = ws.pop("WS_COUNT")
    kept = parse_kept(text)
    bad = []
    for k in kept:
        if k not in ws:
            bad.append("WS_KEPT names %s, which is not a slot" % k)
    for k, v in sorted(ws.items()):
        if not 0 <= v < count:
            bad.append("%s = %d is not below WS_COUNT = %d" % (k, v, count))
        if owner(k) is None:
            bad.append("%s: no entry point of this test takes the prefix (add it to CALLS)" % k)
    if count != max(ws.values()) + 1:
        bad.append("WS_COUNT = %d is not one past the highest slot %d" % (count, max(ws.values())))
    by_value = {}
    for k, v in ws.items():
        by_value.setdefault(v, []).append(k)
    # a kept slot's number: no name of another entry point, and of its own only the named aliases
    for k in kept:
        for other in by_value.get(ws.get(k), []):
            if other == k or frozenset((k, other)) in ALIASES:
                continue
            if owner(other) != owner(k):
                bad.append("kept %s = %d shares its number with %s of another entry point" % (k, ws[k], other))
            else:
                bad.append("kept %s = %d shares its number with %s, which is not a named alias" % (k, ws[k], other))
    # inside one call: a shared number only for the named aliases
    for call, prefixes in CALLS.items():
        names = [k for k in ws if owner(k) is not None and any(k.startswith(p) for p in prefixes)]
        seen = {}
        for k in sorted(names):
            for other in seen.get(ws[k], []):
                if frozenset((k, other)) not in ALIASES:
                    bad.append("%s takes %s and %s, both slot %d" % (call, other, k, ws[k]))
            seen.setdefault(ws[k], []).append(k)
    for a in ALIASES:
        x, y = sorted(a)
        if ws.get(x) is None or ws.get(x) != ws.get(y):
            bad.append("alias %s = %s does not hold" % (x, y))
    pin = parse_enum(text, "PinnedSlot")
    pcount = pin.pop("PINNED_COUNT")
    for k, v in sorted(pin.items()):
        if not 0 <= v < pcount:
            bad.append("%s = %d is not below PINNED_COUNT = %d" % (k, v, pcount))
    if len(set(pin.values())) != len(pin):
        bad.append("two pinned slots share a number")
    return bad


@pytest.fixture(scope="module")
def ctx_h():
    with open(CTX_H) as f:
        return f.read()


def test_slot_table_keeps_its_rules(ctx_h):
    assert slot_violations(ctx_h) == []


def test_the_two_indel_tiles_sharing_a_buffer_is_caught(ctx_h):
    """The checker itself: the numbering in which bcfgpu_pileup_indel_tile and bcfgpu_gap_prep_tile put their tiles in the
    same two slots (each call overwrote the other's tile) breaks the rules."""
    ws = parse_enum(ctx_h, "WsSlot")
    old = re.sub(r"\bWS_GTILE_RECS = \d+", "WS_GTILE_RECS = %d" % ws["WS_ITILE_RECS"], ctx_h)
    old = re.sub(r"\bWS_GTILE_SEL = \d+", "WS_GTILE_SEL = %d" % ws["WS_ITILE_SEL"], old)
    assert old != ctx_h
    bad = slot_violations(old)
    assert any("WS_ITILE_SEL" in b and "WS_GTILE_SEL" in b for b in bad), bad
    assert any("WS_ITILE_RECS" in b and "WS_GTILE_RECS" in b for b in bad), bad
