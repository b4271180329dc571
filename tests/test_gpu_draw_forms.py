"""errmod_cal's replayed draw (bcfgpu_errmod_plan, csrc/draw.hip) in every form of the likelihood kernel: the LDS-histogram
form with the deep cells ranked across workgroups, the global-histogram form, the launch of listed cells (DEEP = true), lists
filled to one below their bound, both passes with many samples, the generator from call to call, the fused pipeline.

Every case asserts (a) the planned result equals the oracle under the draw, (b) the context's generator stands where the
twin's (tests/helpers/drawtwin.py) and the oracle's do, (c) no cell was cut by the first-255 rule, (d) the planned PLs equal the
device's own unplanned PLs of the twin-reduced tile -- a check that does not go through the oracle's draw -- and (e) the draw
differs from the first-255 rule in a deep cell, i.e. the plan mattered.  The tiles and what each is for: tests/helpers/drawtiles.py;
that each holds its regime is asserted in tests/test_oracle_draw_twin.py.  PARITY UNPINNED at the root, as in tests/test_gpu_draw.py."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import drawtiles as dt
from tests.test_gpu_parity import assert_mplp_equal, assert_call_equal

pytestmark = pytest.mark.gpu


def _cut(ctx):
    n = C.c_uint32(77)
    assert ctx.L.bcfgpu_truncated_cells(ctx.h, C.byref(n)) == 0
    return n.value


def _all(checks):
    """Every check is made, so that a failure says which of (a)..(e) hold: [(label, callable)]."""
    bad = []
    for label, f in checks:
        try:
            ok = f()
            assert ok is None or bool(ok)
        except AssertionError as e:
            bad.append("(%s) %s" % (label, " ".join(str(e).split())[:400]))
    assert not bad, "\n".join(bad)


def _check_planned(ctx, c, r):
    got, _ = ctx.mpileup_planned(c.snp)
    state, cut = int(ctx.L.bcfgpu_errmod_state(ctx.h)), _cut(ctx)
    red = ctx.mpileup(r.reduced)
    _all([("a: the oracle under the draw", lambda: assert_mplp_equal(got, r.want)),
          ("b: the generator", lambda: state == r.twin_state == r.orc_state),
          ("c: every deep cell planned, nothing refused", lambda: cut == 0),
          ("d: the device's own PLs of the twin-reduced tile", lambda: np.testing.assert_array_equal(got.pl, red.pl)),
          ("e: the plan mattered", lambda: dt.deep_cells_differ(r.want, r.first, c.deep) > 0)])
    return got


@pytest.mark.parametrize("min_baseQ", [0, 13, 30])
def test_lds_form_ranked_across_workgroups(gpu_ctx_factory, min_baseQ):
    c = dt.lds(min_baseQ)
    assert c.hist_slots <= 8 and len(c.deep) > 256 and c.deep.sum() > 64
    _check_planned(gpu_ctx_factory(c.cfg()), c, dt.refs(c))


def test_global_form_at_the_same_density(gpu_ctx_factory):
    c = dt.glob()
    assert c.hist_slots > 8 and c.deep.sum() > 64
    _check_planned(gpu_ctx_factory(c.cfg()), c, dt.refs(c))


@pytest.mark.parametrize("n_smpl,n_sites,seed", [(300, 1, 61), (40, 3, 62)])
def test_listed_cells_with_a_plan(gpu_ctx_factory, n_smpl, n_sites, seed):
    c = dt.listed(n_smpl, n_sites, seed)
    r = dt.refs(c)
    a, b = c.listed
    assert (c.entries[c.listed] > dt.GLF_MAX_WINDOW).all() and c.deep[a] and not c.deep[b]
    _check_planned(gpu_ctx_factory(c.cfg()), c, r)
    assert dt.deep_cells_differ(r.want, r.first, np.arange(len(c.deep)) == a) == 1      # the plan mattered in the listed cell itself


@pytest.mark.parametrize("n_smpl,n_sites,seed", [(4, 8, 71), (40, 2, 72)])
def test_lists_filled_to_one_below_their_bound(gpu_ctx_factory, n_smpl, n_sites, seed):
    c = dt.filled(n_smpl, n_sites, seed)
    n = len(c.snp.rd)
    cfg = c.cfg()
    assert cfg.max_reads == n and c.deep.all() and c.deep.sum() == n // 256          # `cap` (draw.hip) and `wide_cap` (api.hip) are n / 256 + 1
    _check_planned(gpu_ctx_factory(cfg), c, dt.refs(c))


def test_both_passes_with_many_samples(gpu_ctx_factory):
    c = dt.both()
    r = dt.refs_both(c)
    kept, live = r.kept, r.live
    assert c.hist_slots <= 8 and c.deep.any() and c.i_deep.any() and not live.all() and not c.visit.all()
    ctx = gpu_ctx_factory(c.cfg())
    got_s, got_i = ctx.mpileup_planned(c.snp, c.indel, c.cols, c.ret, visit=c.visit)
    state, cut = int(ctx.L.bcfgpu_errmod_state(ctx.h)), _cut(ctx)
    red_s, red_i = ctx.mpileup(r.reduced), ctx.mpileup(r.reduced_i)
    S = c.n_smpl

    def indel_planes():
        for k in ("pl", "dp4", "adf", "adr", "qs"):
            np.testing.assert_array_equal(getattr(got_i, k)[live], getattr(r.want_i, k)[live], err_msg="indel pass " + k)
        np.testing.assert_array_equal(got_i.site["shift"][live], r.want_i.site["shift"][live])

    _all([("a: the oracle under the draw, SNP pass", lambda: assert_mplp_equal(dt.rows(got_s, kept), r.want)),
          ("a: the oracle under the draw, indel pass", indel_planes),
          ("b: the generator", lambda: state == r.twin_state == r.orc_state),
          ("c: every deep cell planned, nothing refused", lambda: cut == 0),
          ("d: twin-reduced tile, SNP pass", lambda: np.testing.assert_array_equal(got_s.pl[kept], red_s.pl[kept])),
          ("d: twin-reduced tile, indel pass", lambda: np.testing.assert_array_equal(got_i.pl[live], red_i.pl[live])),
          ("e: the plan mattered, SNP pass", lambda: dt.deep_cells_differ(r.want, dt.rows(r.first, kept), c.deep[np.repeat(c.visit != 0, S)]) > 0),
          ("e: the plan mattered, indel pass", lambda: dt.deep_cells_differ(r.want_i, r.first_i, c.i_deep & np.repeat(live, S)) > 0)])


def test_the_generator_goes_on_across_calls(gpu_ctx_factory):
    a, b = dt.lds(13), dt.lds_other()
    ra, rb = dt.refs_chain(a, b)
    ctx = gpu_ctx_factory(a.cfg(max_reads=max(a.max_reads, b.max_reads)))
    _check_planned(ctx, a, ra)
    got = _check_planned(ctx, b, rb)                                                   # the oracle going on with reset=False; the twin's state after both
    assert not np.array_equal(got.pl, dt.refs(b).want.pl)                              # a fresh generator would have drawn other reads


@pytest.mark.parametrize("case", ["lds", "cohort"])
def test_fused_pipeline_with_a_plan(gpu_ctx_factory, case):
    from tests.test_gpu_ctx_state import _pipeline, _call_want
    c = dt.lds(13) if case == "lds" else dt.cohort()
    assert c.n_smpl == 48 or c.n_smpl >= 256                                            # mcall.hip: the `small_too` launch set from 256 samples
    r = dt.refs(c)
    cfg = c.cfg()
    ctx = gpu_ctx_factory(cfg)
    m, call = _pipeline(ctx, c.snp, plan=True)
    state, cut = int(ctx.L.bcfgpu_errmod_state(ctx.h)), _cut(ctx)
    m_red, _ = ctx.pipeline(r.reduced)
    want = _call_want(cfg, r.want)
    _all([("a: the oracle under the draw", lambda: assert_mplp_equal(m, r.want)),
          ("a: orc.mcall on the oracle's planes", lambda: assert_call_equal(call, want, c.n_smpl)),
          ("b: the generator", lambda: state == r.twin_state == r.orc_state),
          ("c: every deep cell planned, nothing refused", lambda: cut == 0),
          ("a called site holds a deep cell", lambda: bool(((want.site["ret"] > 0) & c.deep.reshape(-1, c.n_smpl).any(axis=1)).any())),
          ("d: the device's own PLs of the twin-reduced tile", lambda: np.testing.assert_array_equal(m.pl, m_red.pl)),
          ("e: the plan mattered", lambda: dt.deep_cells_differ(r.want, r.first, c.deep) > 0)])
