"""The oracle's bookkeeping around errmod_cal's draw -- which reads of a cell are usable, their order in bases[], the order in
which a tile's cells take from the one generator -- checked against the plain restatement in tests/helpers/drawtwin.py on every
tile of tests/helpers/drawtiles.py: the generator must stand where the twin's does, and the PLs must be those of the tile the
twin has cut down to the reads it keeps (errmod_cal sorts what it keeps).  Everything but the PLs is over all reads under either
rule.  The regimes the device tests (tests/test_gpu_draw_forms.py) rely on are asserted here, tile by tile.
PARITY UNPINNED at the root, as in tests/test_gpu_draw.py: twin, oracle and device restate htslib's published rules."""
import numpy as np
import pytest

from bcftools_amd import abi
from tests.helpers import drawtiles as dt, drawtwin

SNP_CASES = {
    "lds-Q0": lambda: dt.lds(0), "lds-Q13": lambda: dt.lds(13), "lds-Q30": lambda: dt.lds(30), "lds-other": dt.lds_other,
    "global": dt.glob, "listed-300x1": lambda: dt.listed(300, 1, 61), "listed-40x3": lambda: dt.listed(40, 3, 62),
    "filled-4x8": lambda: dt.filled(4, 8, 71), "filled-40x2": lambda: dt.filled(40, 2, 72), "cohort": dt.cohort,
}


def _same_but_pl(a, b, what):
    for k in dt.PLANES[1:]:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=what + " " + k)
    for k in dt.EXACT_SITE:
        np.testing.assert_array_equal(a.site[k], b.site[k], err_msg=what + " site." + k)


def _same_alleles(a, b, what):
    """The reduced tile's PLs line up with the whole tile's only if bcf_call_combine orders the alleles alike on both."""
    for k in ("a", "n_alleles", "unseen"):
        np.testing.assert_array_equal(a.site[k], b.site[k], err_msg=what + ": the tile is unfit for the comparison, site." + k)


def check_refs(c, r):
    assert r.n_deep == int(c.deep.sum()) > 0
    assert r.orc_state == r.twin_state
    assert (~r.keep).sum() == int((c.n_use[c.deep] - abi.MAX_DEPTH).sum())
    _same_alleles(r.want, r.red, "draw")
    np.testing.assert_array_equal(r.want.pl, r.red.pl, err_msg="PLs under the draw against the twin-reduced tile")
    _same_but_pl(r.want, r.first, "draw against first-255")
    assert dt.deep_cells_differ(r.want, r.first, c.deep) > 0
    assert dt.deep_cells_differ(r.want, r.first, ~c.deep) == 0


@pytest.mark.parametrize("name", sorted(SNP_CASES))
def test_oracle_draw_is_the_twins(name):
    c = SNP_CASES[name]()
    check_refs(c, dt.refs(c))


def test_oracle_goes_on_from_tile_to_tile():
    a, b = dt.lds(13), dt.lds_other()
    ra, rb = dt.refs_chain(a, b)
    check_refs(b, rb)
    assert rb.twin_state != dt.refs(b).twin_state != ra.twin_state           # the second tile drew from where the first stopped
    assert not np.array_equal(rb.want.pl, dt.refs(b).want.pl)


def test_oracle_draw_of_both_passes_is_the_twins():
    c = dt.both()
    r = dt.refs_both(c)
    assert r.orc_state == r.twin_state
    kept, live = r.kept, r.live
    np.testing.assert_array_equal(r.want.pl, r.red.pl[kept])
    np.testing.assert_array_equal(r.want_i.pl[live], r.red_i.pl[live])
    _same_alleles(r.want, dt.rows(r.red, kept), "SNP pass")
    _same_alleles(dt.rows(r.want_i, np.nonzero(live)[0]), dt.rows(r.red_i, np.nonzero(live)[0]), "indel pass")
    _same_but_pl(r.want, dt.rows(r.first, kept), "SNP pass")
    _same_but_pl(dt.rows(r.want_i, np.nonzero(live)[0]), dt.rows(r.first_i, np.nonzero(live)[0]), "indel pass")
    # the cells that drew: the deep ones of the visited columns and of the indel sites whose pass runs
    S = c.n_smpl
    drew_s = c.deep & np.repeat(c.visit != 0, S)
    drew_i = c.i_deep & np.repeat(live, S)
    assert r.n_deep == int(drew_s.sum() + drew_i.sum())
    first_kept = dt.rows(r.first, kept)
    assert dt.deep_cells_differ(r.want, first_kept, drew_s[np.repeat(c.visit != 0, S)]) > 0
    assert dt.deep_cells_differ(r.want_i, r.first_i, drew_i) > 0
    # where the pass does not run the twin keeps the first 255
    assert dt.deep_cells_differ(r.red, r.first, c.deep & ~drew_s) == 0 and (c.deep & ~drew_s).any()
    assert dt.deep_cells_differ(r.red_i, r.first_i, c.i_deep & ~drew_i) == 0 and (c.i_deep & ~drew_i).any()


# ---- what the tiles are for: asserted, so that a change to a generator cannot quietly lose a regime ----

@pytest.mark.parametrize("min_baseQ", [0, 13, 30])
def test_lds_tile_regimes(min_baseQ):
    c = dt.lds(min_baseQ)
    assert c.hist_slots <= 8                                        # the LDS-histogram form
    assert len(c.entries) > 256                                     # two workgroups of draw_scan_kernel
    assert c.deep.sum() >= 70 > 64                                  # two workgroups of draw_shuffle_kernel
    assert c.deep[:256].any() and c.deep[256:].any()
    u = c.n_use[c.deep]
    assert u.min() == 256 and 600 < u.max() <= 700
    big = c.entries > 257
    for n in (255, 256, 257):
        assert ((c.n_use == n) & big).any()
    assert ((c.entries > abi.MAX_DEPTH) & (c.n_use < abi.MAX_DEPTH)).any()
    assert c.deep[0] and c.deep[-1] and (c.deep[:-1] & c.deep[1:] & (np.arange(len(c.deep) - 1) % c.n_smpl != c.n_smpl - 1)).any()
    rd = c.snp.rd
    assert set(np.unique((rd >> 16) & 0xf)) == set(range(16))
    assert {0, 255} <= set(np.unique((rd >> 8) & 0xff))
    q = rd & 0xff
    if min_baseQ:
        assert (q == min_baseQ - 1).any()
    assert (q == min_baseQ).any() or min_baseQ == 0
    for bit in (abi.RD_REV, abi.RD_SCLIP, abi.RD_DEL, abi.RD_SKIP):
        assert 0 < ((rd & bit) != 0).sum() < len(rd)
    ordinary = np.repeat(c.entries < 40, c.entries)
    assert 0.02 < ((rd & abi.RD_DEL) != 0)[ordinary].mean() < 0.05 and 0.01 < ((rd & abi.RD_SKIP) != 0)[ordinary].mean() < 0.035
    assert 8 < c.entries[c.entries < 40].mean() < 16
    assert 15 in c.snp.ref16 and len(rd) < 2e5
    # deletions, ref-skips and low bases all sit inside deep cells: the usable count is not the entry count there
    assert (c.entries[c.deep] > c.n_use[c.deep]).sum() > 30


def test_other_tile_regimes():
    g = dt.glob()
    assert g.hist_slots > 8 and g.deep.sum() >= 70 and len(g.snp.rd) < 2e5
    for c in (dt.listed(300, 1, 61), dt.listed(40, 3, 62)):
        a, b = c.listed
        assert c.hist_slots <= 8 and (c.entries[c.listed] > dt.GLF_MAX_WINDOW).all()
        assert c.deep[a] and not c.deep[b] and c.deep.sum() == 2 and len(c.snp.rd) < 2e5
        r = dt.refs(c)
        assert dt.deep_cells_differ(r.want, r.first, np.arange(len(c.deep)) == a) == 1
    for c in (dt.filled(4, 8, 71), dt.filled(40, 2, 72)):
        n = len(c.snp.rd)
        assert c.deep.all() and c.deep.sum() == n // 256 == (n // 256 + 1) - 1 and c.max_reads == n     # one below `cap` and `wide_cap`
    assert dt.filled(4, 8, 71).hist_slots > 8 >= dt.filled(40, 2, 72).hist_slots
    assert dt.filled(40, 2, 72).deep.sum() > 64
    c = dt.both()
    assert c.hist_slots <= 8 and c.deep.sum() >= 10 and c.i_deep.sum() >= 6
    assert c.deep[2 * c.n_smpl:3 * c.n_smpl].any() and c.visit[2] == 0 and 2 not in c.cols
    assert c.i_deep[c.n_smpl:2 * c.n_smpl].any() and c.ret[1] != 0
    aux, ird = c.indel.aux, c.indel.rd
    assert set(np.unique(aux >> 16)) == {0, 1, 2, 3, 4}
    assert ((aux & 0xff) < 13).any() and ((aux & 0xff) >= 13).any()
    use_i = drawtwin.usable(c.indel, 13)
    assert (use_i & ((ird & abi.RD_DEL) != 0)).any() and (use_i & ((ird & 0xff) < 13)).any()
    assert dt.cohort().n_smpl >= 256 and dt.cohort().deep.sum() >= 20
    assert dt.lds_other().hist_slots <= 8 and dt.lds_other().deep.sum() >= 40
