// mcall_route.h -- which instantiation of mcall_kernel<MAXA, NSUB, ...> works on a site.  Plain C++17, constexpr functions only:
// the kernel, launch_mcall and tests/test_mcall_route.py (a host program) all read the rule from here.
//
// Three instantiations share the grid, every workgroup looks at its site and leaves when the site is another's:
//   (3, 7)   sites of at most three alleles; not launched when `small_too` is set (many samples: nearly every site shows four
//            or five alleles, and the few that do not run in (5, 15) -- same arithmetic, longer loops)
//   (5, 15)  the other sites with at most fifteen allele subsets to visit
//   (5, 25)  the sites with more: five alleles, all with a non-zero frequency (5 + 10 + 10 subsets)
// With sample groups the frequencies are sequential sums over all samples, formed after the split: a grouped site goes to
// (5, 25) by its five alleles alone.  Invariants (tested): every site is taken by exactly one launched instantiation, and
// exactly one launched instantiation writes the record of a site nobody works on (skipped or refused).
#ifndef BCFGPU_MCALL_ROUTE_H
#define BCFGPU_MCALL_ROUTE_H

#ifdef __HIPCC__
#define MCALL_ROUTE_HD __host__ __device__
#else
#define MCALL_ROUTE_HD
#endif

MCALL_ROUTE_HD constexpr bool mcall_launched(int maxa, bool small_too) { return !(small_too && maxa == 3); }

// the instantiation that writes the "skipped" / "refused" record of a site no instantiation works on
MCALL_ROUTE_HD constexpr bool mcall_writes_skip(int maxa, int nsub, bool small_too) { return maxa == 3 || (small_too && nsub == 15); }

// First point, from the site's header alone: false = the site is surely another instantiation's.
MCALL_ROUTE_HD constexpr bool mcall_may_take(int maxa, int nsub, int nals, bool small_too, bool grouped)
{
    if (small_too ? (nals <= 3 && nsub == 25) : (nals <= 3) != (maxa == 3)) return false;
    if (maxa == 5 && grouped && (nals == 5) != (nsub == 25)) return false;
    return true;
}

// Second point, once the frequencies are known: the ungrouped sites of the five-allele instantiations split by whether all five
// alleles have a non-zero frequency (`five_freq`; false for a site of fewer alleles).
MCALL_ROUTE_HD constexpr bool mcall_takes_by_freq(int maxa, int nsub, bool grouped, bool five_freq)
{
    return !(maxa == 5 && !grouped) || five_freq == (nsub == 25);
}

MCALL_ROUTE_HD constexpr bool mcall_takes(int maxa, int nsub, int nals, bool small_too, bool grouped, bool five_freq)
{
    return mcall_may_take(maxa, nsub, nals, small_too, grouped) && mcall_takes_by_freq(maxa, nsub, grouped, five_freq);
}

#endif
