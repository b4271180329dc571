"""Which column gets a record, with everything that decides it at once: targets (`-t`, and `-t ^` which leaves the listed columns
out), gVCF blocks that swallow reference-only records, indel records behind their column's SNP record, and tiles of 64 columns so
that blocks, targets and indel candidates meet tile seams.  host/bcfgpu_sam.c decides it once per tile (record_rule_columns,
record_rule_snps, ind_rec) and five readers follow: the candidate list, errmod_cal's visit plan, the gVCF break bytes, the emit
masks of the device encoders and the record loop.  The device encoders write only the records their mask names and the record loop
takes their offsets by site, so a disagreement would give records another record's sample columns without any error: the output
with --device-text (-O v) / --device-records (-O u) must be the plain output, byte for byte, and so must --prefetch's.  The numbers
of block lines, SNP records and indel records are those of the commit before the rule was merged into one place.  The `^` form
has no indel record to give, whatever the region (17:100-600, 17:1-1000 and 17:1-4200 give the same three numbers: with `^` the
reads are still those that overlap the listed stretch, mpileup.c:198-212, and the data's only indel record lies inside it); the two
cases together have all three kinds."""
import os
import subprocess

import pytest

from tests.test_c_host import _tile_cmd, build_host

pytestmark = pytest.mark.gpu

REGION = "17:100-600"
# targets -> (gVCF block lines, SNP records, indel records) of mpileup.6's inputs (--gvcf 0,2,5) over REGION at --tile 64
COUNTS = {"17:150-400": (15, 2, 1), "^17:150-400": (6, 1, 0)}
assert all(sum(c[i] for c in COUNTS.values()) > 0 for i in range(3))          # not empty output


def _stdout(cmd, extra):
    return subprocess.run(cmd[:1] + extra + cmd[1:], check=True, stdout=subprocess.PIPE).stdout


@pytest.mark.parametrize("targets", sorted(COUNTS))
def test_one_record_rule_for_targets_blocks_and_indels(golden_dir, targets):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    cmd = _tile_cmd(G, "mpileup.6.out", ["--tile", "64", "-t", targets], REGION)
    text = _stdout(cmd, ["-O", "v"])
    assert _stdout(cmd, ["-O", "v", "--prefetch"]) == text
    assert _stdout(cmd, ["-O", "v", "--device-text"]) == text
    bcf = _stdout(cmd, ["-O", "u"])
    assert _stdout(cmd, ["-O", "u", "--prefetch"]) == bcf
    assert _stdout(cmd, ["-O", "u", "--device-records"]) == bcf
    recs = [ln for ln in text.decode().splitlines() if not ln.startswith("#")]
    blocks = sum("MinDP=" in ln for ln in recs)
    indels = sum("\tINDEL;" in ln for ln in recs)
    print("block lines %d, SNP records %d, indel records %d" % (blocks, len(recs) - blocks - indels, indels))
    assert (blocks, len(recs) - blocks - indels, indels) == COUNTS[targets]
