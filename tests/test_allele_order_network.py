"""The allele ordering of combine_kernel (bcftools_amd/csrc/combine.hip, bam2bcf.c:577-632) sorts the four bases by their sums
with five compare-exchanges on (sum, base) pairs instead of the reference's insertion sort, and walks the sorted pairs with a
"stopped here" flag instead of breaking out of a loop over an index array.  Both are stated here once more, statement by
statement as the kernel has them, and compared with the reference's loops over every ordering and every pattern of ties of
four sums, zeros among them, and every reference base (N and the indel pass's "none" included)."""
import itertools

import pytest


def insertion_order(q):
    """bam2bcf.c:577-582: idx sorted ascending by qsum, an element moves down only past a strictly larger sum"""
    idx = [0, 1, 2, 3]
    for i in range(1, 4):
        j = i
        while j > 0 and q[idx[j]] < q[idx[j - 1]]:
            idx[j], idx[j - 1] = idx[j - 1], idx[j]
            j -= 1
    return idx


def network_order(q):
    """combine.hip: CEX(a, b) swaps when (q_b, i_b) < (q_a, i_a); pairs (0,1) (2,3) (0,2) (1,3) (1,2)"""
    p = [[q[i], i] for i in range(4)]

    def cex(a, b):
        if p[b][0] < p[a][0] or (p[b][0] == p[a][0] and p[b][1] < p[a][1]):
            p[a], p[b] = p[b], p[a]
    for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
        cex(a, b)
    return [i for _, i in p]


def reference_walk(q, idx, ref4, ref_base_known):
    """bam2bcf.c:586-611 as the kernel had it: a loop that breaks, idx[i] read behind it"""
    a, qout, unseen = [ref4, -1, -1, -1, -1], [0.0] * 5, -1
    j, i = 1, 3
    while i >= 0:
        ipos = idx[i]
        if ipos == ref4:
            qout[0] = q[ipos]
        else:
            if not q[ipos]:
                break
            qout[j] = q[ipos]
            a[j] = ipos
            j += 1
        i -= 1
    if ref_base_known and ((ref4 < 4 and j < 4) or (ref4 == 4 and j < 5)) and i >= 0:
        unseen = j
        a[j] = idx[i]
        j += 1
    return a, qout, unseen, j


def kernel_walk(q, order, ref4, ref_base_known):
    """combine.hip: the unrolled walk over the sorted pairs"""
    sq, si = [q[i] for i in order], order
    a, qout, unseen = [ref4, -1, -1, -1, -1], [0.0] * 5, -1
    j, stop, stop_base = 1, -1, 0
    for i in (3, 2, 1, 0):
        if stop >= 0:
            continue
        ipos = si[i]
        if ipos == ref4:
            qout[0] = sq[i]
        elif not sq[i]:
            stop, stop_base = i, ipos
        else:
            qout[j] = sq[i]
            a[j] = ipos
            j += 1
    if ref_base_known and ((ref4 < 4 and j < 4) or (ref4 == 4 and j < 5)) and stop >= 0:
        unseen = j
        a[j] = stop_base
        j += 1
    return a, qout, unseen, j


SUMS = [0.0, 0.5, 1.25, 7.0]          # four distinct values, zero among them: 4^4 tuples hold every ordering and every tie pattern


def test_the_network_gives_the_insertion_sort_s_order():
    seen = set()
    for q in itertools.product(SUMS, repeat=4):
        want = insertion_order(q)
        assert network_order(q) == want, q
        seen.add(tuple(want))
    assert len(seen) == 24                  # every permutation of the four bases came out


@pytest.mark.parametrize("ref4,known", [(0, True), (1, True), (2, True), (3, True), (4, True), (0, False)])
def test_the_unrolled_walk_gives_the_loop_s_alleles(ref4, known):
    stops, runs_through = 0, 0
    for q in itertools.product(SUMS, repeat=4):
        want = reference_walk(q, insertion_order(q), ref4, known)
        assert kernel_walk(q, network_order(q), ref4, known) == want, (q, ref4)
        stops += want[2] >= 0
        runs_through += want[3] == 5 or (want[2] < 0 and known)
    assert not known or (stops and runs_through)
