"""bcfgpu_call's prior: the allele count it derives from the ploidy definition, and -P.

The reference fills every sample's ploidy with ploidy_max() of the definition before mcall_init (vcfcall.c:652-656), so the prior
counts n = ploidy_max * samples alleles (mcall.c:396-416): samples with `--ploidy 1` or a definition that is `* * * * 1` alone,
twice the samples without a definition, with --ploidy X / Y / GRCh37, and with every definition whose largest line or default is 2
(ploidy.c:109-110, 122-131, 259-262).  A record whose QUAL is the prior alone (mcall.c:1641-1642, tests/helpers/priorrecs.py)
shows n without any likelihood arithmetic: the driver's QUAL there must be the closed form.  -P theta is compared record by record
with the test-side driver over the oracle.  The driver has no CPU path: all of this needs the GPU."""
import os
import subprocess

import pytest

from bcftools_amd import abi
from tests.helpers import orc, vcf, calldrv as D, priorrecs as PR
from tests.test_c_host import CALL_EXE, VIEW_EXE, build_host
from tests.test_c_host_device_input import cohort  # noqa: F401  (the 70-sample fixture)

pytestmark = pytest.mark.gpu

NAMES = ["s1", "s2", "s3"]
POS0 = 101
THETA = 1.1e-3                       # call's default -P (vcfcall.c:943)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """(directory, in.vcf, in.bcf, positions of the prior-only records): a dozen records of three samples."""
    build_host()
    d = tmp_path_factory.mktemp("prior")
    cin, where = PR.records(31, 40, len(NAMES), False)
    others = [k for k in PR.representable(cin) if k not in where][:12 - len(where)]
    idx = sorted(others + where.tolist())
    assert len(idx) == 12
    sub = PR.select(cin, idx)
    at = [idx.index(k) for k in where]
    # on the CPU: the records take the route in the oracle, and others among them are called as variants
    res = orc.mcall(abi.default_cfg(len(NAMES)), sub)
    PR.assert_prior_only(res, at)
    assert (res.site["als_new"] != 1).sum() >= 2
    src, bcf = str(d / "in.vcf"), str(d / "in.bcf")
    PR.write_vcf(sub, src, NAMES, POS0)
    subprocess.check_call([VIEW_EXE, "-O", "u", "-o", bcf, src])
    (d / "one.txt").write_text("* * * * 1\n")
    (d / "sexes.txt").write_text("* * * M 1\n* * * F 1\n")
    (d / "one_and_two.txt").write_text("* * * * 1\nX 1 100 M 2\n")
    # --ploidy Y makes the default sex (the last one named, F) absent: without a sex of their own no sample would be called and
    # QUAL would be missing (no REF allele counted, mcall.c:1643-1644)
    (d / "sexes.samples").write_text("s1\tM\ns2\tF\ns3\tM\n")
    return d, src, bcf, [POS0 + k for k in at]


def call(args, src, tmp):
    """The driver's output as (bytes, tests.helpers.vcf.Vcf); BCF output goes through bcfgpu_view."""
    p = subprocess.run([CALL_EXE] + list(args) + [src], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr
    text = p.stdout
    if "u" in args or "b" in args:
        text = subprocess.run([VIEW_EXE, "-"], input=text, check=True, stdout=subprocess.PIPE).stdout
    f = os.path.join(str(tmp), "out.vcf")
    with open(f, "wb") as fh:
        fh.write(text)
    return p.stdout, vcf.Vcf(f)


def assert_prior_only_qual(out, at, theta, n):
    want = float(PR.prior_only_qual(theta, n))
    recs = {r.pos: r for r in out.recs}
    for pos in at:
        r = recs[pos]
        assert r.alts == [] and r.qual is not None, r.line
        assert abs(r.qual - want) <= D.qual_tol(want), (pos, r.qual, want, n)


@pytest.mark.parametrize("args,n", [
    ("-m --ploidy 1", 3), ("-m --ploidy-file {D}/one.txt", 3),
    ("-m", 6), ("-m --ploidy X", 6), ("-m --ploidy Y -S {D}/sexes.samples", 6), ("-m --ploidy GRCh37", 6),
    ("-m --ploidy-file {D}/sexes.txt", 6), ("-m --ploidy-file {D}/one_and_two.txt", 6)])
def test_prior_counts_ploidy_max_alleles_a_sample(inputs, tmp_path, args, n):
    d, src, bcf, at = inputs
    assert abs(float(PR.prior_only_qual(THETA, 3)) - float(PR.prior_only_qual(THETA, 6))) > 100 * D.qual_tol(27.0)
    _, out = call(args.format(D=str(d)).split(), src, tmp_path)
    assert len(out.recs) == 12
    assert_prior_only_qual(out, at, THETA, n)


@pytest.mark.parametrize("theta", ["0", "0.01", "0.9"])
def test_prior_option_matches_the_twin_over_the_oracle(inputs, tmp_path, theta):
    d, src, bcf, at = inputs
    _, out = call(["-m", "-P", theta], src, tmp_path)
    called, names = D.run_call(vcf.Vcf(src), orc.mcall, theta=float(theta))
    assert len(called) == 12
    D.compare_with_golden(called, names, out)
    assert_prior_only_qual(out, at, float(theta), 6)
    if float(theta) == 0:
        assert all(r.qual == 0 for r in out.recs if r.pos in at)
    # -P moves the records: the default's output is another
    _, dflt = call(["-m"], src, tmp_path)
    assert [r.qual for r in dflt.recs] != [r.qual for r in out.recs]


def test_prior_and_haploid_definition_on_a_cohort(cohort, tmp_path):  # noqa: F811
    """-P 0.2 --ploidy 1 on 70 samples: theta' stays under the cap for 70 alleles and would not for 140."""
    d, bcf = cohort
    assert not PR.scaled_theta(0.2, 70)[1] and PR.scaled_theta(0.2, 140)[1]
    text = subprocess.run([VIEW_EXE, bcf], check=True, stdout=subprocess.PIPE).stdout
    src = str(tmp_path / "cohort.vcf")
    with open(src, "wb") as fh:
        fh.write(text)
    one = str(tmp_path / "one.txt")
    open(one, "w").write("* * * * 1\n")
    pl = D.parse_ploidy_file(one)
    assert D.ploidy_max(pl) == 1
    _, out = call(["-P", "0.2", "--ploidy", "1"], bcf, tmp_path)
    v = vcf.Vcf(src)
    called, names = D.run_call(v, orc.mcall, theta=0.2, ploidy=pl, ploidy_max=1)
    assert len(called) >= 200
    D.compare_with_golden(called, names, out)
    # ... and the allele count shows in this cohort's records: with 2 alleles a sample the twin gives other QUALs
    twice, _ = D.run_call(v, orc.mcall, theta=0.2, ploidy=pl, ploidy_max=2)
    assert sum(abs(a.qual - b.qual) > 10 * D.qual_tol(b.qual) for a, b in zip(twice, called)) >= 10


@pytest.mark.parametrize("opt,use_bcf,mode", [("--device-input", True, "v"), ("--device-parse", False, "v"), ("--device-records", True, "u")])
def test_device_routes_carry_the_same_prior(inputs, tmp_path, opt, use_bcf, mode):
    d, src, bcf, at = inputs
    args = ["-O", mode, "--ploidy", "1"]
    plain, out = call(args, bcf if use_bcf else src, tmp_path)
    dev, _ = call([opt] + args, bcf if use_bcf else src, tmp_path)
    assert dev == plain
    assert_prior_only_qual(out, at, THETA, 3)
