"""The staged read pool: bcfgpu_pool_stage brings the next region's pool to the device beside the context's pool, and
bcfgpu_pool_adopt makes it the context's pool.  After the adopt the context must be what bcfgpu_pool_upload of the same arrays
leaves, and until then nothing about the current pool may change.  Every comparison is byte equality against the same calls
on a fresh context with bcfgpu_pool_upload; no test asserts a time."""
import ctypes as C
import os

import numpy as np
import pytest

from bcftools_amd import abi, engine, synth
from bcftools_amd.lib import check, load
from tests.helpers import sam, mplpdrv as M
from tests.test_gpu_ctx_state import _cfg, _gap_prep_tile, _host, _mplp, PLANES
from tests.test_gpu_pileup import assert_tiles_equal

pytestmark = pytest.mark.gpu

FORMS = ("plain", "packed0", "packed2", "packed4", "recs")
PER_READ = ("r_pos", "r_lq", "r_flag", "r_ncig", "r_cig_off", "r_seq_off")


class Pool:
    """A region's reads as the caller's host arrays in one of the input forms of bcfgpu_pool_upload: plain (a byte per base);
    packed0/2/4 (4-bit bases; qualities a byte each, or 2- / 4-bit palette indices); recs (packed4 with 12-byte read records).
    pinned: the arrays lie in page-locked memory (bcfgpu_host_alloc)."""

    def __init__(self, reads, mapq, smpl, ref, form="plain", pinned=False):
        self.n, self.nb, self.form = int(reads["n_reads"]), len(reads["qual"]), form
        self.smpl, self.ref = np.ascontiguousarray(smpl, dtype=np.int32), ref
        self._pinned = []
        a = {k: reads[k] for k in PER_READ + ("cig",)}
        a["mapq"] = np.ascontiguousarray(mapq, dtype=np.uint8)
        qual = reads["qual"]
        self.palette = None
        if form == "plain":
            a["seq16"], a["qual"] = reads["seq16"], qual
        else:
            a["seq4"] = abi.pack_nibbles(reads["seq16"])
            if form == "packed0":
                a["qual"] = qual
            else:
                self.palette = np.unique(qual)
                bits = 2 if form == "packed2" else 4
                assert len(self.palette) <= (1 << bits)
                a["qual4"] = (abi.pack_crumbs if bits == 2 else abi.pack_nibbles)(np.searchsorted(self.palette, qual).astype(np.uint8))
            if form == "recs":
                lq = reads["r_lq"].astype(np.int64)
                assert (lq % 4 == 0).all() and (reads["r_seq_off"] == np.r_[0, np.cumsum(lq)[:-1]]).all()       # dense, as records need
                a["recs"] = abi.read12(reads["r_pos"], reads["r_lq"], reads["r_ncig"], reads["r_flag"], a["mapq"]).view(np.uint8)
                for k in PER_READ + ("mapq",):
                    del a[k]
        self.a = {k: (self._pin(v) if pinned else np.array(v, copy=True)) for k, v in a.items()}
        self.n_cig = len(reads["cig"])

    def _pin(self, v):
        L, p = load(), C.c_void_p()
        check(L.bcfgpu_host_alloc(max(v.nbytes, 1), C.byref(p)))
        self._pinned.append(p)
        w = np.ctypeslib.as_array((C.c_uint8 * max(v.nbytes, 1)).from_address(p.value))[:v.nbytes].view(v.dtype)
        w[...] = v
        return w

    def free(self):
        L = load()
        self.a = {}
        for p in self._pinned:
            check(L.bcfgpu_host_free(p))
        self._pinned = []

    def args(self):
        """(bcfgpu_reads, bcfgpu_packed or None, r_mapq) over the arrays; the structs are kept alive on self."""
        a = self.a
        rd = abi.Reads()
        rd.n_reads = self.n
        for k in PER_READ + ("cig", "seq16", "qual"):
            if k in a:
                setattr(rd, k, a[k].ctypes.data)
        pk = None
        if self.form != "plain":
            pk = abi.Packed()
            pk.seq4, pk.n_bases, pk.n_cig = a["seq4"].ctypes.data, self.nb, self.n_cig
            if "qual4" in a:
                pk.qual4, pk.qual_bits = a["qual4"].ctypes.data, 2 if self.form == "packed2" else 4
                for j, q in enumerate(self.palette):
                    pk.palette[j] = int(q)
            if "recs" in a:
                pk.recs = a["recs"].ctypes.data
        self._structs = (rd, pk)
        return C.byref(rd), (C.byref(pk) if pk is not None else None), (a["mapq"].ctypes.data if "mapq" in a else None)

    def scribble(self):
        """Other bytes in every host array (what a caller does once the arrays are its own again)."""
        for v in self.a.values():
            v.view(np.uint8)[...] = 0xA5


def upload(ctx, pool):
    check(ctx.L.bcfgpu_pool_upload(ctx.h, *pool.args()))


def stage(ctx, pool):
    check(ctx.L.bcfgpu_pool_stage(ctx.h, *pool.args()))


def adopt(ctx):
    check(ctx.L.bcfgpu_pool_adopt(ctx.h))


def synth_pool(seed, n_sites, S, depth, form="plain", pinned=False, bins4=False, **kw):
    b = synth.indel_batch(seed, n_sites, S, depth=depth, **kw)
    reads, mapq, smpl, _ = synth.indel_pool(b)
    mapq = mapq.copy()
    mapq[::5] = 37                                                 # (not one value: the records carry it per read)
    if bins4:                                                      # four quality bins, as a 2-bit palette needs
        q = reads["qual"].copy()
        q[q == 2] = 11
        q[q == 41] = 40
        reads = dict(reads, qual=q)
    p = Pool(reads, mapq, smpl, b["ref"], form, pinned)
    p.b = b
    return p


def short_chain(ctx, pool, beg=0, end=None):
    """BAQ -> overlap tweak -> pileup -> download on the context's pool (which is `pool`): every output as bytes."""
    L, n = ctx.L, pool.n
    ref = pool.ref
    end = len(ref) if end is None else end
    ret = np.full(n, 99, np.int32)
    check(L.bcfgpu_pool_baq(ctx.h, ref, len(ref), 3, ret.ctypes.data))
    pa, pb = np.arange(0, n - 1, 2, dtype=np.int32)[:32], np.arange(1, n, 2, dtype=np.int32)[:32]
    check(L.bcfgpu_pool_overlap_tweak(ctx.h, len(pa), pa.ctypes.data if len(pa) else None, pb.ctypes.data if len(pb) else None))
    t = abi.Tile()
    col_n, col_indel = np.zeros(end - beg, np.int32), np.zeros(end - beg, np.uint8)
    check(L.bcfgpu_pool_pileup(ctx.h, pool.smpl.ctypes.data if n else None, None, beg, end, ref, len(ref), C.byref(t),
                               col_n.ctypes.data, col_indel.ctypes.data))
    tile = _host(ctx, t)
    q, z, m = np.zeros(pool.nb, np.uint8), np.zeros(pool.nb, np.uint8), np.zeros(n, np.uint8)
    check(L.bcfgpu_pool_download(ctx.h, q.ctypes.data, z.ctypes.data, m.ctypes.data))
    return dict(ret=ret, col_n=col_n, col_indel=col_indel, qual=q, zq=z, mapq=m, tile=tile)


def full_chain(ctx, pool):
    """A region as host/bcfgpu_sam.c runs a tile, on the context's pool (which is `pool`): BAQ, the -C cap, the keep mask, the
    overlap tweak, the pileup, bcfgpu_gap_prep_tile on the candidate columns (ZQ from HBM), bcfgpu_errmod_plan_visit and both
    bcfgpu_mpileup passes."""
    L, n, b = ctx.L, pool.n, pool.b
    ref = pool.ref
    check(L.bcfgpu_pool_baq(ctx.h, ref, len(ref), 3, None))
    cap = np.zeros(n, np.int32)
    check(L.bcfgpu_pool_cap_mapq(ctx.h, ref, len(ref), 50, cap.ctypes.data))
    keep = (cap >= 0).astype(np.uint8)
    keep[::13] = 0
    check(L.bcfgpu_pool_keep(ctx.h, keep.ctypes.data))
    pa, pb = np.arange(0, n - 1, 2, dtype=np.int32)[:32], np.arange(1, n, 2, dtype=np.int32)[:32]
    check(L.bcfgpu_pool_overlap_tweak(ctx.h, len(pa), pa.ctypes.data, pb.ctypes.data))
    q, z, m = np.zeros(pool.nb, np.uint8), np.zeros(pool.nb, np.uint8), np.zeros(n, np.uint8)
    check(L.bcfgpu_pool_download(ctx.h, q.ctypes.data, z.ctypes.data, m.ctypes.data))
    t = abi.Tile()
    col_n = np.zeros(len(ref), np.int32)
    check(L.bcfgpu_pool_pileup(ctx.h, pool.smpl.ctypes.data, None, 0, len(ref), ref, len(ref), C.byref(t), col_n.ctypes.data, None))
    g, gt = _gap_prep_tile(ctx, ref, b["pos"], col_n)
    assert len(g["live_cols"]) > 0
    visit = np.ones(int(t.n_sites), np.uint8)
    visit[::7] = 0
    visit[g["live_cols"]] = 1
    check(L.bcfgpu_errmod_plan_visit(ctx.h, C.byref(t), visit.ctypes.data, C.byref(gt), g["live_cols"].ctypes.data, None))
    return dict(cap=cap, qual=q, zq=z, mapq=m, col_n=col_n, g_ret=g["ret"], g_aux=g["aux"], g_types=g["types"],
                tile=_host(ctx, t), snp=_mplp(ctx, t), gtile=_host(ctx, gt), indel=_mplp(ctx, gt))


def assert_same(got, want):
    assert got.keys() == want.keys()
    for k, w in want.items():
        g = got[k]
        if isinstance(w, np.ndarray):
            assert g.tobytes() == w.tobytes(), k
        elif hasattr(w, "plp_off"):                                # a tile
            assert_tiles_equal(g, w)
            assert (g.aux is None) == (w.aux is None) and (w.aux is None or g.aux.tobytes() == w.aux.tobytes()), k
        else:                                                      # bcfgpu_mpileup's planes
            for p in PLANES:
                assert getattr(g, p).tobytes() == getattr(w, p).tobytes(), (k, p)


def alone(S, pool, chain):
    with engine.Context(_cfg(S)) as ctx:
        upload(ctx, pool)
        return chain(ctx, pool)


# ---- stage + adopt is an upload ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "page-locked"])
@pytest.mark.parametrize("form", FORMS)
def test_stage_and_adopt_give_what_upload_gives(form, pinned):
    S = 5
    want = alone(S, synth_pool(301, 9, S, 18.0, form, bins4=True), short_chain)
    assert want["tile"].rd.size > 500 and (want["ret"] == 0).any() and want["zq"].any() and want["col_indel"].any()
    pool = synth_pool(301, 9, S, 18.0, form, pinned, bins4=True)
    with engine.Context(_cfg(S)) as ctx:
        stage(ctx, pool)
        adopt(ctx)
        pool.scribble()                                            # the arrays are the caller's again
        assert_same(short_chain(ctx, pool), want)
    pool.free()
    if form != "plain":                                            # and every form holds the same pool
        assert_same(want, alone(S, synth_pool(301, 9, S, 18.0, "plain", bins4=True), short_chain))


def test_stage_and_adopt_on_the_sam_fixtures(golden_dir):
    """The reference's own reads (soft clips, every CIGAR operation, unsorted samples across files), plain and packed."""
    G = os.path.join(golden_dir, "mpileup")
    sams = [sam.Sam(os.path.join(G, f)) for f in ("mpileup.1.sam", "mpileup.2.sam", "mpileup.3.sam")]
    prep = M.Prepared(sams, sam.read_fasta(os.path.join(G, "mpileup.ref.fa")), "17", sam.MplpOpts(), baq=False, overlaps=False)
    S = len(prep.samples)
    by_sample = [[] for _ in range(S)]
    for rl in prep.files:
        for r, si in rl:
            by_sample[si].append(r)
    flat = [r for rl in by_sample for r in rl]
    smpl = np.array([si for si, rl in enumerate(by_sample) for _ in rl], np.int32)
    _, d = M.pack_reads(flat)
    reads = dict(n_reads=len(flat), **{k: d[k] for k in PER_READ + ("cig", "seq16", "qual")})
    mapq = np.array([r.mapq for r in flat], np.uint8)
    ref = prep.refseq.encode()
    for form in ("plain", "packed0"):
        chain = lambda ctx, pool: short_chain(ctx, pool, 0, 700)
        want = alone(S, Pool(reads, mapq, smpl, ref, form), chain)
        assert want["tile"].rd.size > 1000
        pool = Pool(reads, mapq, smpl, ref, form)
        with engine.Context(_cfg(S)) as ctx:
            stage(ctx, pool)
            adopt(ctx)
            pool.scribble()
            assert_same(chain(ctx, pool), want)


# ---- a staged pool does not disturb the current one; regions in a row -----------------------------------------------------------
def test_regions_in_a_row_each_staged_under_the_one_before():
    """The loop the call exists for: stage region i + 1, run region i's whole chain, adopt.  The read counts go up, down, to
    zero reads and up again, so that both sets of the pool's slots and the staging slots regrow while the other role is in
    use; one region has cells past 255 reads; the forms alternate.  Every region gives what it gives alone."""
    S = 4
    spec = [(401, 6, 12.0, "plain", {}), (402, 20, 30.0, "recs", {}), (403, 4, 8.0, "packed4", {}), None,
            (404, 3, 320.0, "plain", dict(max_depth=450)), (405, 12, 25.0, "packed0", {}), (406, 5, 10.0, "recs", {})]

    def make(sp, pinned):
        if sp is None:
            p = Pool(dict(n_reads=0, qual=np.zeros(0, np.uint8), seq16=np.zeros(0, np.uint8), cig=np.zeros(0, np.uint32),
                          **{k: np.zeros(0, np.int32) for k in PER_READ}), np.zeros(0, np.uint8), np.zeros(0, np.int32), b"ACGTACGTACGT")
            p.b = None
            return p
        seed, n_sites, depth, form, kw = sp
        return synth_pool(seed, n_sites, S, depth, form, pinned, **kw)

    def chain(ctx, pool):
        return short_chain(ctx, pool) if pool.b is None else full_chain(ctx, pool)
    want = [alone(S, make(sp, False), chain) for sp in spec]
    assert want[3]["tile"].rd.size == 0
    deep = want[4]["tile"]
    assert (np.diff(deep.plp_off.astype(np.int64)) > 255).any()
    pools = [make(sp, i % 2 == 0) for i, sp in enumerate(spec)]
    with engine.Context(_cfg(S)) as ctx:
        upload(ctx, pools[0])
        for i, pool in enumerate(pools):
            if i + 1 < len(pools):
                stage(ctx, pools[i + 1])
            assert_same(chain(ctx, pool), want[i])                 # with the next pool's copies in flight or landed
            if i + 1 < len(pools):
                adopt(ctx)
                pools[i + 1].scribble()
    for p in pools:
        p.free()


def test_large_pools_alternate_under_each_others_stages():
    """Pools of 2e5-3e5 reads (tens of megabytes an array: copies that last while kernels run), page-locked and pageable, in a
    ring: each is staged while BAQ, the tweak and the pileup of the other run, and is later overwritten by the next stage while
    its successor's kernels are still queued behind it."""
    S = 420
    A, B = synth_pool(77, 24, S, 30.0, "plain", pinned=True), synth_pool(78, 16, S, 30.0, "recs", pinned=False)
    assert A.n > 2.5e5 and B.n > 1.5e5
    want = {id(A): alone(S, A, short_chain), id(B): alone(S, B, short_chain)}
    with engine.Context(_cfg(S)) as ctx:
        upload(ctx, A)
        cur, nxt = A, B
        for _ in range(4):
            stage(ctx, nxt)
            assert_same(short_chain(ctx, cur), want[id(cur)])
            adopt(ctx)
            cur, nxt = nxt, cur
        assert_same(short_chain(ctx, cur), want[id(cur)])
    A.free()


def test_a_second_stage_replaces_the_first():
    S = 4
    A, B = synth_pool(411, 10, S, 20.0, "recs"), synth_pool(412, 5, S, 12.0, "plain")
    want = alone(S, synth_pool(412, 5, S, 12.0, "plain"), full_chain)
    with engine.Context(_cfg(S)) as ctx:
        stage(ctx, A)
        stage(ctx, B)
        adopt(ctx)
        assert_same(full_chain(ctx, B), want)
        assert ctx.L.bcfgpu_pool_adopt(ctx.h) == abi.E_ARG         # one adopt per stage


def test_adopt_with_nothing_staged_is_refused_and_the_pool_stays():
    S = 4
    A = synth_pool(421, 6, S, 15.0)
    want = alone(S, synth_pool(421, 6, S, 15.0), full_chain)
    with engine.Context(_cfg(S)) as ctx:
        assert ctx.L.bcfgpu_pool_adopt(ctx.h) == abi.E_ARG         # not even a pool
        upload(ctx, A)
        assert ctx.L.bcfgpu_pool_adopt(ctx.h) == abi.E_ARG
        msg = ctx.L.bcfgpu_last_error()
        assert b"bcfgpu_pool_adopt" in msg and b"no staged read pool" in msg and b"bcfgpu_pool_stage" in msg
        assert_same(full_chain(ctx, A), want)


def test_stage_checks_its_arguments_as_upload_does():
    S = 4
    A = synth_pool(422, 4, S, 10.0)
    with engine.Context(_cfg(S)) as ctx:
        upload(ctx, A)
        rd, _, mapq = A.args()
        codes = []
        for fn in (ctx.L.bcfgpu_pool_upload, ctx.L.bcfgpu_pool_stage):
            bad = abi.Reads()
            bad.n_reads = A.n                                      # reads without arrays
            pk = abi.Packed()
            pk.qual_bits = 3
            codes.append((fn(ctx.h, None, None, mapq), fn(ctx.h, C.byref(bad), None, mapq), fn(ctx.h, rd, None, None), fn(ctx.h, rd, C.byref(pk), mapq)))
        assert codes[0] == codes[1] == (abi.E_ARG,) * 4
        assert ctx.L.bcfgpu_pool_adopt(ctx.h) == abi.E_ARG         # a refused stage stages nothing


def test_after_adopt_the_old_pileup_is_refused_as_after_upload():
    S = 4
    A, B = synth_pool(431, 6, S, 15.0), synth_pool(432, 4, S, 10.0)
    codes = []
    for how in ("upload", "adopt"):
        with engine.Context(_cfg(S)) as ctx:
            upload(ctx, A)
            r = full_chain(ctx, A)
            if how == "upload":
                upload(ctx, B)
            else:
                stage(ctx, B)
                cols = np.ascontiguousarray(A.b["pos"], dtype=np.int32)
                n = int(r["col_n"][cols].sum())
                so, e = np.zeros(len(cols) * S + 1, np.int32), np.zeros(n, np.int32)
                check(ctx.L.bcfgpu_pileup_entries(ctx.h, len(cols), cols.ctypes.data, so.ctypes.data, e.ctypes.data, e.ctypes.data, e.ctypes.data, n))
                adopt(ctx)                                         # (a stage alone took nothing away)
            cols = np.ascontiguousarray(A.b["pos"], dtype=np.int32)
            n = int(r["col_n"][cols].sum())
            so, e = np.zeros(len(cols) * S + 1, np.int32), np.zeros(n, np.int32)
            rc = ctx.L.bcfgpu_pileup_entries(ctx.h, len(cols), cols.ctypes.data, so.ctypes.data, e.ctypes.data, e.ctypes.data, e.ctypes.data, n)
            codes.append((rc, b"gone" in ctx.L.bcfgpu_last_error()))
            with pytest.raises(engine.BcfGpuError) as err:
                _gap_prep_tile(ctx, A.ref, cols, r["col_n"])
            codes.append((err.value.code, "gone" in str(err.value)))
    assert codes[0] == codes[2] == (abi.E_ARG, True) and codes[1] == codes[3] == (abi.E_ARG, True)


def test_on_the_callers_stream():
    import torch
    S = 4
    A, B = synth_pool(441, 8, S, 15.0, "recs", pinned=True), synth_pool(442, 14, S, 25.0, "plain", pinned=True)
    want = [alone(S, synth_pool(441, 8, S, 15.0, "recs"), full_chain), alone(S, synth_pool(442, 14, S, 25.0, "plain"), full_chain)]
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    with engine.Context(_cfg(S)) as ctx:
        check(ctx.L.bcfgpu_set_stream(ctx.h, C.c_void_p(st.cuda_stream)))
        stage(ctx, A)
        adopt(ctx)
        stage(ctx, B)
        assert_same(full_chain(ctx, A), want[0])
        adopt(ctx)
        B.scribble()
        assert_same(full_chain(ctx, B), want[1])
        st.synchronize()
    A.free()
    B.free()


def test_destroy_with_a_staged_pool_pending():
    S = 4
    A, B = synth_pool(451, 6, S, 15.0), synth_pool(452, 30, S, 40.0, "recs", pinned=True)
    want = alone(S, synth_pool(451, 6, S, 15.0), full_chain)
    with engine.Context(_cfg(S)) as ctx:
        upload(ctx, A)
        stage(ctx, B)
    B.free()                                                       # destroy has waited for the copies
    with engine.Context(_cfg(S)) as ctx:
        upload(ctx, A)
        assert_same(full_chain(ctx, A), want)
