"""`bcfgpu_call -g INT,...`: every spelling of the option -- `-g 0` behind `-m`, `-g0`, `-mg0` (test.pl:277) and `--gvcf 0` --
goes through one parser (parse_gvcf_limits of host/drv.h) and gives the same bytes; `-mg0` gives the reference's golden; what is
not a list of at most 16 integers ends the run with exit code 1 and the message that names the argument as it was given (the
glued `-mg...` form names it from its third character on).  `bcfgpu_sam --gvcf` keeps its own limit message."""
import os
import subprocess

import pytest

from tests.test_c_host import CALL_EXE, SAM_EXE, build_host, whole_file_checks

pytestmark = pytest.mark.gpu

SEVENTEEN = ",".join(str(i) for i in range(17))


def _stdout(args, vcf):
    return subprocess.run([CALL_EXE] + args + [vcf], check=True, stdout=subprocess.PIPE).stdout


@pytest.mark.parametrize("limits", ["0", "0,2,5"])
def test_every_spelling_of_the_gvcf_option_gives_the_same_bytes(golden_dir, limits):
    build_host()
    vcf = os.path.join(golden_dir, "call", "mpileup.vcf")
    outs = [_stdout(args, vcf) for args in (["-m", "-g", limits], ["-g" + limits], ["-mg" + limits], ["--gvcf", limits])]
    assert all(o == outs[0] for o in outs[1:])
    recs = [ln for ln in outs[0].splitlines() if not ln.startswith(b"#")]
    assert recs and any(b"MinDP=" in ln for ln in recs)


def test_glued_gvcf_option_gives_the_golden(golden_dir):
    build_host()
    G = os.path.join(golden_dir, "call")
    whole_file_checks([CALL_EXE, "-mg0", os.path.join(G, "mpileup.vcf")], os.path.join(G, "mpileup.2.out"))


@pytest.mark.parametrize("args,message", [
    (["-g", "x"], "Could not parse: --gvcf x\n"),
    (["-gx"], "Could not parse: --gvcf x\n"),
    (["-mgx"], "Could not parse: --gvcf gx\n"),
    (["-g", SEVENTEEN], "Could not parse: --gvcf " + SEVENTEEN + "\n"),
])
def test_bad_gvcf_limits_end_the_caller(golden_dir, args, message):
    build_host()
    p = subprocess.run([CALL_EXE] + args + [os.path.join(golden_dir, "call", "mpileup.vcf")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", message)


def test_too_many_gvcf_limits_end_the_mpileup_driver(golden_dir):
    build_host()
    G = os.path.join(golden_dir, "mpileup")
    p = subprocess.run([SAM_EXE, "--gvcf", SEVENTEEN, "-f", os.path.join(G, "mpileup.ref.fa"), "-r", "17:100-110", os.path.join(G, "mpileup.1.sam")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "--gvcf: at most 16 limits\n")
