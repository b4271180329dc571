"""Where the sites of five alleles lie in a tile.  The instantiations of mcall_kernel (bcftools_amd/csrc/mcall.hip) share one grid
and each site is taken by exactly one of them, chosen from its allele count and frequencies.  The fused pipeline writes five
alleles only where the reference base is N, so the N positions are what the cases place: at the first and the last of 64
consecutive sites, in a ragged last 64, all 64 of one run and none of the next, a tile of one site, and no N at all --
ungrouped (such a site's reference allele has no frequency: the 15-subset instantiation keeps it), with four sample groups
(the 25-subset one takes it) and with a ploidy array.  bcfgpu_pipeline against the oracle, as
tests/test_gpu_parity.py::test_subset_scan_corners."""
import numpy as np
import pytest

from bcftools_amd import abi, host, synth
from tests.helpers import orc
from tests.test_gpu_parity import assert_call_equal, assert_mplp_equal

pytestmark = pytest.mark.gpu

PLACEMENTS = {
    "one_site": (1, [0]),
    "lane_edges": (130, [0, 63, 64, 127, 128, 129]),
    "a_whole_wavefront": (192, list(range(64, 128))),
    "no_n": (130, []),
}


@pytest.mark.parametrize("mode", ["ungrouped", "groups", "ploidy"])
@pytest.mark.parametrize("n_smpl", [40, 300])
@pytest.mark.parametrize("place", list(PLACEMENTS))
def test_n_reference_sites_wherever_they_lie(gpu_ctx_factory, place, n_smpl, mode):
    n_sites, n_at = PLACEMENTS[place]
    seed = 9100 + 7 * list(PLACEMENTS).index(place) + n_smpl
    tile = synth.numpy_tile(seed, n_sites, n_smpl, depth=12.0, var_rate=0.6, wide_qual=True)
    tile.ref16[n_at] = 15
    n_grp = 4 if mode == "groups" else 1
    fmt = abi.INFO_VDB | abi.INFO_RPB | (abi.FMT_AD if n_grp > 1 else 0)
    kw = dict(n_grp=n_grp) if n_grp > 1 else {}
    cfg = abi.default_cfg(n_smpl, max_sites=n_sites, max_reads=len(tile.rd), fmt_flag=fmt, **kw)
    rng = np.random.default_rng(seed)
    ploidy = rng.choice([1, 2, 2], size=n_smpl).astype(np.uint8) if mode == "ploidy" else None
    grp = None
    if n_grp > 1:
        grp = (np.arange(n_smpl) * n_grp // n_smpl).astype(np.int32)
        rng.shuffle(grp)
    mwant = orc.mpileup(cfg, tile)
    na = mwant.site["n_alleles"]
    # the case is what it says: five alleles at the N sites and nowhere else (unbinned qualities: with 300 samples every base is
    # seen at every site; with 40 some N sites show fewer and stay with the other instantiations)
    five = set(np.nonzero(na == 5)[0].tolist())
    assert five <= set(n_at) and (n_smpl == 40 or five == set(n_at))
    ad = None
    if n_grp > 1:
        src = mwant.adf.astype(np.int32) + mwant.adr.astype(np.int32)
        ad = np.where(np.arange(5)[None, :, None] < na[:, None, None], src, abi.INT32_VECTOR_END).astype(np.int32)
    cin = host.CallInput(n_smpl, na, np.maximum(mwant.site["unseen"], 0), mwant.pl.astype(np.int32), mwant.site["qsum"],
                         ad=ad, ploidy=ploidy, grp=grp, i16=mwant.site["anno"].astype(np.float32))
    cwant = orc.mcall(cfg, cin)
    mgot, cgot = gpu_ctx_factory(cfg).pipeline(tile, ploidy=ploidy, grp=grp)
    assert_mplp_equal(mgot, mwant)
    assert_call_equal(cgot, cwant, n_smpl)
    if n_sites > 1:
        assert (cwant.site["nals_new"] > 1).any()
