"""`bcfgpu_sam --prefetch`: the pool of tile i + 1 goes to the device (bcfgpu_pool_stage, from page-locked buffers) while the
device stages of tile i run, and tile i + 1 starts with bcfgpu_pool_adopt.  The output must be the output without the option,
byte for byte, and the reference's goldens, whole files, as VCF and through BCF: many tiles and few, gVCF blocks carried over
tile seams, indel candidates at tile edges, -B (the current tile's host arrays are read by bcfgpu_gap_prep_tile while the next
tile's are being filled), region shards."""
import os
import subprocess

import pytest

from tests.test_c_host import SAM_EXE, _tile_cmd, build_host, whole_file_checks

pytestmark = pytest.mark.gpu


def _same_with_and_without(cmd):
    """cmd (without --prefetch) and cmd with it: the same bytes on stdout; returns them."""
    plain = subprocess.run(cmd, check=True, stdout=subprocess.PIPE).stdout
    pre = subprocess.run(cmd[:1] + ["--prefetch"] + cmd[1:], check=True, stdout=subprocess.PIPE).stdout
    assert pre == plain
    return plain


@pytest.mark.parametrize("tile", [64, 1000])
@pytest.mark.parametrize("goldf", ["mpileup.2.out", "mpileup.11.out"])
def test_prefetch_many_tiles_and_few(golden_dir, goldf, tile):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    cmd = _tile_cmd(G, goldf, ["--tile", str(tile)])
    whole_file_checks(cmd[:1] + ["--prefetch"] + cmd[1:], os.path.join(G, goldf))
    assert len(_same_with_and_without(cmd)) > 10000


@pytest.mark.parametrize("tile", [37, 128])
def test_prefetch_carries_gvcf_blocks_across_tiles(golden_dir, tile):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    cmd = _tile_cmd(G, "mpileup.6.out", ["--tile", str(tile)])
    whole_file_checks(cmd[:1] + ["--prefetch"] + cmd[1:], os.path.join(G, "mpileup.6.out"))
    _same_with_and_without(cmd)
    # and over the seam of two regions (the staged tile is run before the next region starts)
    cmd = _tile_cmd(G, "mpileup.6.out", ["--tile", str(tile)], "17:100-257,17:258-600")
    whole_file_checks(cmd[:1] + ["--prefetch"] + cmd[1:], os.path.join(G, "mpileup.6.out"))


@pytest.mark.parametrize("tile", [64, 512])
def test_prefetch_indel_records_over_every_sequence(golden_dir, tile):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    cmd = _tile_cmd(G, "indel-AD.1.out", ["--tile", str(tile)])
    whole_file_checks(cmd[:1] + ["--prefetch"] + cmd[1:], os.path.join(G, "indel-AD.1.out"))
    _same_with_and_without(cmd)


def test_prefetch_without_baq(golden_dir):
    """-B: no BAQ, so bcfgpu_gap_prep_tile takes the ZQ tags from the tile's host pool -- which must still be that tile's
    while the next tile's pool is built and staged.  The golden with -B (a few columns: tiles of four), and a contig with
    indel records, with and without the option."""
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    cmd = [SAM_EXE, "--prefetch", "--tile", "4", "-B", "--ff", "0x14", os.path.join(G, "mpileup.ref.fa"), "17", "1050", "1060", os.path.join(G, "mpileup.1.sam")]
    whole_file_checks(cmd, os.path.join(G, "mpileup.3.out"))
    for tile in (64, 1000):
        out = _same_with_and_without(_tile_cmd(G, "mpileup.11.out", ["-B", "--tile", str(tile)]))
        assert out.count(b"INDEL;") > 0
    _same_with_and_without(_tile_cmd(G, "indel-AD.1.out", ["-B", "--tile", "64"]))


@pytest.mark.parametrize("goldf", ["mpileup.11.out", "mpileup.6.out"])
def test_prefetch_in_region_shards(golden_dir, goldf):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    cmd = _tile_cmd(G, goldf, ["--gpus", "2", "--tile", "128"])
    whole_file_checks(cmd[:1] + ["--prefetch"] + cmd[1:], os.path.join(G, goldf))
    _same_with_and_without(cmd)


def test_prefetch_with_the_mapq_cap_and_timing(golden_dir):
    """-C 50 (the side context that caps mapping qualities runs a tile ahead) and --timing, whose line names the wait inside
    bcfgpu_pool_adopt."""
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    cmd = _tile_cmd(G, "mpileup.11.out", ["-C", "50", "--tile", "256"])
    _same_with_and_without(cmd)
    p = subprocess.run(cmd[:1] + ["--prefetch", "--timing"] + cmd[1:], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"bcfgpu_pool_adopt" in p.stderr
