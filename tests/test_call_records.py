"""The plain statement of the gather's call records (tests/helpers/callrec.py) checked on the CPU: its header layout against
include/bcfgpu.h as the host compiler lays it out, and walk(pack(...)) giving back the selected sites' planes."""
import os
import subprocess

import numpy as np
import pytest

from bcftools_amd import abi, host
from tests.helpers import callrec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "bcfgpu.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(bcfgpu_call_rec), offsetof(bcfgpu_call_rec, call), offsetof(bcfgpu_call_rec, mplp),
           offsetof(bcfgpu_call_rec, site), offsetof(bcfgpu_call_rec, n_gt), offsetof(bcfgpu_call_rec, bytes));
    return 0;
}
"""


def test_rec_dtype_is_the_headers_layout(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_call, o_mplp, o_site, o_ngt, o_bytes = (int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split())
    assert (size, o_call, o_mplp) == (400, 16, 128) and size % 16 == 0
    d = callrec.REC_DTYPE
    assert d.itemsize == size
    assert [d.fields[k][1] for k in ("site", "n_gt", "bytes", "pad", "call", "mplp")] == [o_site, o_ngt, o_bytes, 12, o_call, o_mplp]
    assert d.fields["call"][0] == host.CALLSITE_DTYPE and d.fields["mplp"][0] == host.SITE_DTYPE


def synthetic_calls(seed, n_sites, n_smpl, n_gt_planes, with_msite=True):
    """Call planes as no caller would leave them but as the compaction may meet them: ret from -2 .. 5, nals_new = ret when
    ret > 0 else 0, pl_dropped set for every one-allele record and for about one in ten of the others, every other header field
    random, GT random bytes, PL random words with both sentinels among them.  Returns (call_site, gt, pl, msite or None)."""
    rng = np.random.default_rng(seed)
    cs = np.frombuffer(rng.integers(0, 256, n_sites * host.CALLSITE_DTYPE.itemsize, dtype=np.uint8).tobytes(), host.CALLSITE_DTYPE).copy()
    ret = rng.integers(-2, 6, n_sites).astype(np.int32)
    ret[:min(n_sites, 8)] = np.arange(-2, 6)[:min(n_sites, 8)]             # every value is there when the tile has eight sites
    cs["ret"] = ret
    cs["nals_new"] = np.where(ret > 0, ret, 0)
    cs["pl_dropped"] = ((cs["nals_new"] == 1) | (rng.random(n_sites) < 0.1)).astype(np.int32)
    if n_sites >= 16:                                                       # one dropped-PL record with alleles, one skipped record with and one without the flag
        cs["pl_dropped"][8:11] = 1
        cs["ret"][8:11], cs["nals_new"][8:11] = (3, 0, 0), (3, 0, 0)
        cs["pl_dropped"][10] = 0
    gt = rng.integers(-128, 128, (n_sites, 2, n_smpl)).astype(np.int8)
    pl = rng.integers(-2**31, 2**31, (n_sites, n_gt_planes, n_smpl)).astype(np.int32)
    pl[rng.random(pl.shape) < 0.05] = abi.INT32_MISSING
    pl[rng.random(pl.shape) < 0.05] = abi.INT32_VECTOR_END
    ms = None
    if with_msite:
        ms = np.frombuffer(rng.integers(0, 256, n_sites * host.SITE_DTYPE.itemsize, dtype=np.uint8).tobytes(), host.SITE_DTYPE).copy()
    return cs, gt, pl, ms


def assert_case_is_telling(cs, variants_only):
    """A case cannot pass vacuously: it drops a site, keeps a record with PL planes, keeps one without and, in mode 0, keeps a
    record of a skipped site."""
    keep = callrec.selected(cs, variants_only)
    ngt = np.array([callrec.n_gt_of(c) for c in cs])
    assert (~keep).any() and (keep & (ngt > 0)).any() and (keep & (ngt == 0)).any()
    if variants_only == 0:
        assert (keep & (cs["nals_new"] == 0)).any()


@pytest.mark.parametrize("variants_only", [0, 1, 2])
@pytest.mark.parametrize("n_smpl", [1, 2, 3, 5])
def test_walk_gives_back_what_pack_was_given(n_smpl, variants_only):
    n_sites, planes, site0 = 64, 15, 1000
    cs, gt, pl, ms = synthetic_calls(100 + n_smpl, n_sites, n_smpl, planes)
    assert_case_is_telling(cs, variants_only)
    buf, n_rec = callrec.pack(cs, gt, pl, n_smpl, planes, site0, variants_only, ms)
    recs = callrec.walk(buf, n_smpl)
    want = np.nonzero(callrec.selected(cs, variants_only))[0]
    assert n_rec == len(recs) == len(want)
    # the selection, stated once more site by site
    for k in range(n_sites):
        r, nn = int(cs["ret"][k]), int(cs["nals_new"][k])
        assert (k in want) == (r >= 0 and not (variants_only >= 1 and r == 0) and not (variants_only == 2 and nn < 2))
    o = 0
    for (h, g, p), k in zip(recs, want):
        nn = int(cs["nals_new"][k])
        ng = 0 if cs["pl_dropped"][k] else nn * (nn + 1) // 2
        assert int(h["site"]) == site0 + k and int(h["n_gt"]) == ng and int(h["pad"]) == 0
        assert h["call"].tobytes() == cs[k].tobytes() and h["mplp"].tobytes() == ms[k].tobytes()
        np.testing.assert_array_equal(g, gt[k] if nn else np.full((2, n_smpl), abi.GT_MISSING, np.int8))
        np.testing.assert_array_equal(p, pl[k, :ng])
        # the gaps are zero: between the GT block and the PL block, and behind the PL block
        size, g_end = int(h["bytes"]), 400 + 2 * n_smpl
        pl0 = 400 + (2 * n_smpl + 3) // 4 * 4
        assert pl0 - g_end == (-2 * n_smpl) % 4 and size == (pl0 + 4 * ng * n_smpl + 15) // 16 * 16
        assert not any(buf[o + g_end:o + pl0]) and not any(buf[o + pl0 + 4 * ng * n_smpl:o + size])
        o += size
    assert o == len(buf)


def test_pack_without_site_records_leaves_them_zero():
    cs, gt, pl, _ = synthetic_calls(7, 20, 3, 15, with_msite=False)
    buf, n_rec = callrec.pack(cs, gt, pl, 3, 15, 0, 0)
    recs = callrec.walk(buf, 3)
    assert n_rec == len(recs) > 0 and all(not any(h["mplp"].tobytes()) for h, _, _ in recs)


def test_walk_refuses_a_truncated_buffer():
    cs, gt, pl, ms = synthetic_calls(8, 20, 2, 15)
    buf, _ = callrec.pack(cs, gt, pl, 2, 15, 0, 0, ms)
    with pytest.raises(AssertionError):
        callrec.walk(buf[:-16], 2)
