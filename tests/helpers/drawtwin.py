"""errmod_cal's draw over a tile, restated plainly: which 255 reads every cell of more than 255 usable reads keeps, from the
published rules alone (bam2bcf.c:170-203 for the reads that reach bases[], mpileup.c:330-360 for the order in which
mpileup_reg() meets the cells, htslib ksort.h ks_shuffle and os/rand.c hts_drand48 for the draw).  The generator's state is a
Python integer; nothing here calls the oracle or the device library, so it stands beside both (csrc/draw.hip,
oracle/bam2bcf_oracle.c + oracle/errmod.c) as a third statement of the same rules.

errmod_cal sorts the reads it keeps, so a tile from which the reads a deep cell does not keep are taken out (`reduced`) has,
under any rule, the PLs that the draw must give on the whole tile."""
import numpy as np

from bcftools_amd import abi, host

SEED = 0x1234ABCD330E
_A, _C, _M = 0x5DEECE66D, 0xB, (1 << 48) - 1
_TWO48 = float(1 << 48)


def usable(tile, min_baseQ=13):
    """The entries of a tile that reach bases[]: the SNP pass drops ref-skips, deletions and bases under min_baseQ
    (bam2bcf.c:173, :187, :192); the indel pass drops ref-skips only (a low indelQ turns the read into a REF read, :183)."""
    rd = tile.rd
    u = (rd & np.uint32(abi.RD_SKIP)) == 0
    if not tile.is_indel:
        u &= (rd & np.uint32(abi.RD_DEL)) == 0
        u &= (rd & np.uint32(0xff)).astype(np.int64) >= int(min_baseQ)
    return u


def _cell(tile, site, s, use, keep, x, run):
    """One errmod_cal call: a cell of n > 255 usable reads keeps 255 of them -- by ks_shuffle if the cell is visited (`run`),
    else the first 255.  Returns (generator state, 1 if the cell drew)."""
    c = site * tile.n_smpl + s
    b, e = int(tile.plp_off[c]), int(tile.plp_off[c + 1])
    if e - b <= abi.MAX_DEPTH:
        return x, 0
    a = [i for i in range(b, e) if use[i]]
    n = len(a)
    if n <= abi.MAX_DEPTH:
        return x, 0
    if run:
        for i in range(n, 1, -1):
            x = (_A * x + _C) & _M
            j = int(x / _TWO48 * i)                          # (int)(hts_drand48() * i), in double as ksort.h does it
            a[j], a[i - 1] = a[i - 1], a[j]
    keep[a[abi.MAX_DEPTH:]] = False
    return x, 1 if run else 0


def draw(snp, indel=None, cols=None, ret=None, visit=None, min_baseQ=13, state=SEED):
    """Replays the draw over one tile's two passes.  snp, indel: HostTiles (indel may be None); cols: the SNP-tile column of
    every indel site (ascending); ret: bcf_call_gap_prep's return per indel site (None: all 0); visit: per SNP column, 0 = the
    position is passed over before bcf_call_glfgen (None: all visited).
    Returns ((keep mask of the SNP tile, keep mask of the indel tile or None), the generator afterwards, the number of cells that drew).
    A keep mask is False exactly at the usable reads a deep cell does not keep."""
    x, n_deep = int(state), 0
    use_s, keep_s = usable(snp, min_baseQ), np.ones(len(snp.rd), bool)
    use_i = keep_i = None
    at = {}
    if indel is not None:
        use_i, keep_i = usable(indel, min_baseQ), np.ones(len(indel.rd), bool)
        cols = [int(c) for c in cols]
        assert cols == sorted(set(cols)) and len(cols) == indel.n_sites
        at = {c: i for i, c in enumerate(cols)}
    for k in range(snp.n_sites):
        run = visit is None or bool(visit[k])
        for s in range(snp.n_smpl):
            x, d = _cell(snp, k, s, use_s, keep_s, x, run)
            n_deep += d
        if k in at:
            i = at[k]
            run = ret is None or int(ret[i]) == 0
            for s in range(indel.n_smpl):
                x, d = _cell(indel, i, s, use_i, keep_i, x, run)
                n_deep += d
    return (keep_s, keep_i), x, n_deep


def reduced(tile, keep):
    """The tile without the reads that `keep` drops: plp_off, rd, epos and aux follow."""
    keep = np.asarray(keep, bool)
    before = np.r_[0, np.cumsum(keep)]
    return host.HostTile(tile.n_smpl, tile.ref16, before[tile.plp_off.astype(np.int64)].astype(np.uint32), tile.rd[keep], tile.epos[keep],
                         None if tile.aux is None else tile.aux[keep], tile.is_indel)
