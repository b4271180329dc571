"""bench.py --dump-outputs DIR: what the timed path computed in its last step, as float32 / float64 .npy files of at most 64 MB
in all, every value finite, the same from run to run with the same arguments (the inputs are seeded), and --steps the number of
timed steps."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--gpus", "1", "--warmup", "1", "--sites", "2048", "--samples", "200", "--cpu-seconds", "0", "--cpu-all-cores", "0", "--extras", "0"]


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + COMMON + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stderr or r.stdout)[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    a, b = str(d / "a"), str(d / "b")
    return a, _bench(["--steps", "2", "--dump-outputs", a]), b, _bench(["--steps", "3", "--dump-outputs", b])


def test_dump_outputs_are_the_last_steps_and_repeat(dumps):
    a, ja, b, jb = dumps
    assert ja["steps"] == 2 and jb["steps"] == 3 and ja["ms_per_step"] > 0 and jb["ms_per_step"] > 0
    fa = sorted(os.path.basename(f) for f in glob.glob(os.path.join(a, "*.npy")))
    assert fa == sorted(os.path.basename(f) for f in glob.glob(os.path.join(b, "*.npy")))
    assert {"site_index.npy", "mplp_site_depth.npy", "mplp_pl.npy", "call_site_qual.npy", "call_gt.npy", "call_pl.npy",
            "records_counts.npy", "records_bytes.npy"} <= set(fa)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in fa) <= 64_000_000
    for f in fa:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype in (np.float32, np.float64) and x.dtype == y.dtype, f
        assert np.isfinite(x).all(), f                            # HUGE_VAL / NaN of the site records: 0 and a class in <name>_nonfinite
        assert np.array_equal(x, y), f                            # each step recomputes the same tile: the last one is every one
    counts = np.load(os.path.join(a, "records_counts.npy"))
    assert counts[1] == ja["config"]["records_per_step_per_gpu"] > 0 and counts[0] == ja["config"]["record_bytes_per_step_per_gpu"]
    assert len(np.load(os.path.join(a, "site_index.npy"))) == 2048          # a small tile: every site record
    assert (np.load(os.path.join(a, "mplp_site_depth.npy")) > 0).any()
    for f in ("mplp_site_mwu_bq", "mplp_site_vdb", "mplp_site_anno", "call_site_qual"):
        code = np.load(os.path.join(a, f + "_nonfinite.npy"))
        assert code.shape == np.load(os.path.join(a, f + ".npy")).shape and set(np.unique(code)) <= {0, 1, 2, 3}
    assert (np.load(os.path.join(a, "mplp_site_mwu_bq_nonfinite.npy")) == 2).any()     # untested sites: +HUGE_VAL in the record


def test_plain_run_reports_the_headline_only():
    """Without --full and without the options that switch them off, no CPU baseline and no child measurements run."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--sites", "2048",
                        "--samples", "200"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stderr or r.stdout)[-2000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["steps"] == 2 and j["warmup"] == 1 and j["value"] > 0 and j["ms_per_step"] > 0 and j["unit"] == "sites/s"
    assert "cpu_baseline" not in j and "extra" not in j and "configs4_shape_sites_per_s" not in j["config"]


def _columns(tile, sites):
    """the columns `sites` of a HostTile, as a HostTile of their own"""
    from bcftools_amd import host
    S = tile.n_smpl
    off = tile.plp_off.astype(np.int64)
    cells = (np.asarray(sites, np.int64)[:, None] * S + np.arange(S)[None, :]).ravel()
    n = off[cells + 1] - off[cells]
    idx = np.concatenate([np.arange(off[c], off[c + 1]) for c in cells]).astype(np.int64)
    return host.HostTile(S, tile.ref16[sites], np.concatenate([[0], np.cumsum(n)]).astype(np.uint32), tile.rd[idx], tile.epos[idx])


def test_dump_outputs_equal_the_oracle_at_the_dumped_sites(dumps):
    """The dumped planes and records against the CPU oracle on the same seeded tile (bench.py's defaults: seed, depth, variant
    rate), column by column at the dumped sites: plane offsets, layouts and the site index are checked against an independent
    source, and the rows the kernels do not write for a site's alleles are zero."""
    import torch
    from bcftools_amd import abi, host, synth
    from tests.helpers import orc
    a = dumps[0]
    ld = lambda f: np.load(os.path.join(a, f + ".npy"))
    T, S = 2048, 200
    sites, psites = ld("site_index").astype(np.int64), ld("plane_site_index").astype(np.int64)
    assert np.array_equal(sites, np.arange(T)) and len(psites) > 100 and np.all(np.diff(psites) > 0)
    tile = synth.tile_from_torch(synth.torch_tile(20260104, T, S, torch.device("cuda", 0), depth=30.0, var_rate=0.01))
    sub = _columns(tile, psites)
    cfg = abi.default_cfg(S, max_sites=len(psites), max_reads=len(sub.rd), fmt_flag=abi.INFO_VDB | abi.INFO_RPB)
    m = orc.mpileup(cfg, sub)
    c = orc.mcall(cfg, host.CallInput(S, m.site["n_alleles"], np.maximum(m.site["unseen"], 0), m.pl.astype(np.int32), m.site["qsum"],
                                      i16=m.site["anno"].astype(np.float32)))
    np.testing.assert_array_equal(ld("mplp_pl"), m.pl)
    np.testing.assert_array_equal(ld("mplp_dp4"), m.dp4)
    for f in ("n_alleles", "depth", "ori_ref"):
        np.testing.assert_array_equal(ld("mplp_site_" + f)[psites], m.site[f])
    np.testing.assert_array_equal(ld("call_gt"), c.gt)
    np.testing.assert_array_equal(ld("call_pl"), c.pl)
    for f in ("ret", "nals_new", "an", "dp4"):
        np.testing.assert_array_equal(ld("call_site_" + f)[psites], c.site[f])
    assert (c.site["als_new"] != 1).any()                          # a variant site among the compared ones
    # the PL rows past a site's n(n+1)/2 genotypes and the DP4 of a site without alleles: never written, zero
    nal = ld("mplp_site_n_alleles")[psites].astype(np.int64)
    pl = ld("mplp_pl")
    for k, n in enumerate(nal):
        assert not pl[k, n * (n + 1) // 2:].any(), psites[k]
        if n == 0:
            assert not ld("mplp_dp4")[k].any()
