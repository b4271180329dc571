"""The call records of the ordered gather (bcfgpu_call_rec and what follows it) stated in numpy, from the contract in
include/bcfgpu.h ("several GPUs: region shards and the ordered gather"), not from the kernel:

    record   = head (site, n_gt, bytes, pad = 0), the site's bcfgpu_call_site, its bcfgpu_site (zero when none was given),
               GT [2][S] i8, zeros up to a multiple of 4, PL [n_gt][S] i32, zeros up to a multiple of 16
    n_gt     = nals_new (nals_new + 1) / 2, or 0 when pl_dropped
    selected = ret >= 0; variants_only 1: also ret != 0; variants_only 2: also nals_new >= 2
    GT of a record with nals_new == 0 (a site the caller skipped: it wrote no genotype there) is BCFGPU_GT_MISSING throughout

pack() builds the bytes record by record with tobytes(); walk() reads them back.  Nothing here is vectorised or shares a
formula with bcftools_amd/csrc/gather.hip."""
import numpy as np

from bcftools_amd import abi, host

REC_DTYPE = np.dtype([("site", "<i4"), ("n_gt", "<i4"), ("bytes", "<u4"), ("pad", "<i4"),
                      ("call", host.CALLSITE_DTYPE), ("mplp", host.SITE_DTYPE)], align=True)


def selected(call_site, variants_only):
    """bool [n_sites]: the sites whose record is written under `variants_only`"""
    ret, nn = call_site["ret"], call_site["nals_new"]
    keep = ret >= 0
    if variants_only >= 1:
        keep = keep & (ret != 0)
    if variants_only == 2:
        keep = keep & (nn >= 2)
    return keep


def n_gt_of(cs):
    nn = int(cs["nals_new"])
    return 0 if int(cs["pl_dropped"]) else nn * (nn + 1) // 2


def pack(call_site, gt, pl, n_smpl, n_gt_planes, site0, variants_only, msite=None):
    """The records of a tile: call_site [n] CALLSITE_DTYPE, gt [n][2][S] i8, pl [n][n_gt_planes][S] i32, msite [n] SITE_DTYPE or
    None.  Returns (bytes, n_rec)."""
    n = len(call_site)
    gt = np.asarray(gt, np.int8).reshape(n, 2, n_smpl)
    pl = np.asarray(pl, np.int32).reshape(n, n_gt_planes, n_smpl)
    keep = selected(call_site, variants_only)
    out, n_rec = [], 0
    for k in range(n):
        if not keep[k]:
            continue
        ng = n_gt_of(call_site[k])
        assert ng <= n_gt_planes
        g = gt[k] if int(call_site[k]["nals_new"]) else np.full((2, n_smpl), abi.GT_MISSING, np.int8)
        body = g.tobytes()
        body += b"\0" * (-len(body) % 4)
        body += pl[k, :ng].astype("<i4").tobytes()
        h = np.zeros(1, REC_DTYPE)
        size = REC_DTYPE.itemsize + len(body)
        size += -size % 16
        h["site"], h["n_gt"], h["bytes"] = site0 + k, ng, size
        h["call"] = call_site[k]
        if msite is not None:
            h["mplp"] = msite[k]
        rec = h.tobytes() + body
        out.append(rec + b"\0" * (size - len(rec)))
        n_rec += 1
    return b"".join(out), n_rec


def walk(buf, n_smpl):
    """[(header as a REC_DTYPE scalar, gt [2][S] i8, pl [n_gt][S] i32)] of the records in buf; the walk must end at len(buf)."""
    buf = np.frombuffer(bytes(buf), np.uint8)
    H, o, recs = REC_DTYPE.itemsize, 0, []
    while o < len(buf):
        assert o + H <= len(buf), "a record's header passes the end of the buffer"
        h = buf[o:o + H].view(REC_DTYPE)[0]
        ng, size = int(h["n_gt"]), int(h["bytes"])
        pl0 = H + (2 * n_smpl + 3) // 4 * 4
        assert size % 16 == 0 and pl0 + 4 * ng * n_smpl <= size < pl0 + 4 * ng * n_smpl + 16 and o + size <= len(buf), (o, size, ng)
        gt = buf[o + H:o + H + 2 * n_smpl].view(np.int8).reshape(2, n_smpl)
        pl = buf[o + pl0:o + pl0 + 4 * ng * n_smpl].view("<i4").reshape(ng, n_smpl)
        recs.append((h, gt, pl))
        o += size
    assert o == len(buf)
    return recs
