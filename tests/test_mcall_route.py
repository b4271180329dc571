"""The routing rule of the caller's instantiations (bcftools_amd/csrc/mcall_route.h), enumerated on the CPU by a host program:
every site is taken by exactly one launched instantiation of mcall_kernel<MAXA, NSUB, ...>, and exactly one launched
instantiation writes the record of a site nobody works on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INST = [(3, 7), (5, 15), (5, 25)]

ROUTE_CPP = r"""
#include <cstdio>
#include "mcall_route.h"
static_assert(mcall_takes(5, 25, 5, false, false, true), "the header's functions are constant expressions");
int main()
{
    const int inst[3][2] = {{3, 7}, {5, 15}, {5, 25}};
    for (int small_too = 0; small_too < 2; ++small_too)
        for (int nals = 1; nals <= 5; ++nals)
            for (int grouped = 0; grouped < 2; ++grouped)
                for (int five = 0; five < ((nals == 5 && !grouped) ? 2 : 1); ++five) {
                    std::printf("%d %d %d %d", small_too, nals, grouped, five);
                    // per instantiation: launched, writes the skip record, may take (first point), takes
                    for (int i = 0; i < 3; ++i)
                        std::printf("  %d %d %d %d", (int)mcall_launched(inst[i][0], small_too != 0),
                                    (int)mcall_writes_skip(inst[i][0], inst[i][1], small_too != 0),
                                    (int)mcall_may_take(inst[i][0], inst[i][1], nals, small_too != 0, grouped != 0),
                                    (int)mcall_takes(inst[i][0], inst[i][1], nals, small_too != 0, grouped != 0, five != 0));
                    std::printf("\n");
                }
    return 0;
}
"""


def test_every_site_has_one_instantiation(tmp_path):
    src, exe = tmp_path / "route.cpp", tmp_path / "route"
    src.write_text(ROUTE_CPP)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "bcftools_amd", "csrc"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    # nals 1..4: grouped or not; nals 5: grouped, or ungrouped with / without five frequencies; all with and without small_too
    assert len(lines) == 2 * (4 * 2 + 3)
    seen = set()
    for line in lines:
        v = [int(x) for x in line.split()]
        small_too, nals, grouped, five = v[:4]
        seen.add((small_too, nals, grouped, five))
        per = {INST[i]: dict(zip(("launched", "writes", "may", "takes"), v[4 + 4 * i:8 + 4 * i])) for i in range(3)}
        launched = [k for k in INST if per[k]["launched"]]
        assert launched == ([(5, 15), (5, 25)] if small_too else INST), line
        takers = [k for k in launched if per[k]["takes"]]
        writers = [k for k in launched if per[k]["writes"]]
        assert len(takers) == 1, line
        assert len(writers) == 1, line
        # who takes a site has not left at the first point, and a grouped site is settled there
        assert per[takers[0]]["may"], line
        if grouped:
            assert [k for k in launched if per[k]["may"]] == takers, line
            assert (takers[0] == (5, 25)) == (nals == 5), line
        else:
            assert (takers[0] == (5, 25)) == bool(five), line
        if nals <= 3:
            assert takers[0] == ((5, 15) if small_too else (3, 7)), line
        else:
            assert takers[0][0] == 5, line
    assert len(seen) == len(lines)
