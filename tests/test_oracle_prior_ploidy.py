"""The oracle's prior under cfg.ploidy_max (oracle/mcall_oracle.c:576-587; mcall.c:396-416 with vcfcall.c:652-656): the CPU half of
tests/test_gpu_prior_ploidy.py.  The records of tests/helpers/priorrecs.py whose QUAL is the prior alone must take that route
in the oracle -- a change to the generator must not lose it quietly -- and their QUAL must be the closed form in
n = ploidy_max * samples, for ploidy_max 0 (= 2), 1 and 2, one to 65 samples, the default prior, none, and one large enough for the
0.99 cap; with and without a ploidy array.  The twin of bcfgpu_call's ploidy_max rule is checked against the reference's rule
(ploidy.c:109-110, 122-131, 259-262) on the definitions `call` carries with it."""
import numpy as np
import pytest

from bcftools_amd import abi
from tests.helpers import orc, priorrecs as PR, calldrv as D

QUAL_TOL = 1e-4                       # assert_call_equal's tolerance on QUAL (tests/test_gpu_parity.py)
THETAS = [1.1e-3, 0.0, 0.2]
SAMPLES = [1, 2, 3, 65]
N_RANDOM = 12


def cfg_for(n_smpl, theta, ploidy_max, max_sites=0, max_reads=0):
    cfg = abi.default_cfg(n_smpl, max_sites=max_sites, max_reads=max_reads, call_theta=theta)
    cfg.ploidy_max = ploidy_max
    return cfg


def oracle_calls(n_smpl, theta, use_ploidy):
    """(CallInput, the prior-only records, {ploidy_max: oracle CallResult})"""
    cin, where = PR.records(100 + n_smpl, N_RANDOM, n_smpl, use_ploidy)
    return cin, where, {pm: orc.mcall(cfg_for(n_smpl, theta, pm), cin) for pm in (0, 1, 2)}


def check_closed_form(res, where, theta, n_smpl):
    """QUAL at the prior-only records of {ploidy_max: CallResult}: the closed form; 0 equals 2; 1 differs from 2 from two samples
    up and equals it with one; no prior: 0."""
    for pm, r in res.items():
        want = PR.prior_only_qual(theta, PR.prior_alleles(pm, n_smpl))
        np.testing.assert_allclose(r.site["qual"][where], want, rtol=QUAL_TOL, atol=QUAL_TOL, err_msg="ploidy_max %d" % pm)
        assert (r.site["qual_missing"][where] == 0).all()
    np.testing.assert_array_equal(res[0].site["qual"], res[2].site["qual"])
    q1, q2 = res[1].site["qual"][where], res[2].site["qual"][where]
    if theta > 0 and n_smpl >= 2:
        assert (np.abs(q1 - q2) > 100 * QUAL_TOL).all(), (q1, q2)
    else:
        np.testing.assert_array_equal(q1, q2)
    if theta == 0:
        assert (q1 == 0).all() and (q2 == 0).all()


def test_closed_form_figures():
    """The figures the closed form gives for the default prior and three samples, and the cap case: theta = 0.2 with 65 samples
    stays under 1 for 65 alleles and not for 130."""
    assert abs(float(PR.prior_only_qual(1.1e-3, 3)) - 27.8255) < 1e-3 and abs(float(PR.prior_only_qual(1.1e-3, 6)) - 26.0007) < 1e-3
    assert PR.prior_only_qual(1.1e-3, 1) == PR.prior_only_qual(1.1e-3, 2)
    assert PR.scaled_theta(0.2, 65)[1] is False and PR.scaled_theta(0.2, 130)[1] is True
    assert PR.prior_only_qual(0.2, 130) == np.float32(-4.343 * np.log(0.99)) and PR.prior_only_qual(0.2, 65) > PR.prior_only_qual(0.2, 130)
    assert PR.prior_only_qual(0.0, 6) == 0


@pytest.mark.parametrize("use_ploidy", [False, True])
@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("n_smpl", SAMPLES)
def test_oracle_prior_only_records_follow_the_closed_form(n_smpl, theta, use_ploidy):
    cin, where, res = oracle_calls(n_smpl, theta, use_ploidy)
    assert len(where) >= 4 and set(cin.nals[where].tolist()) == {1, 2}
    for r in res.values():
        PR.assert_prior_only(r, where)
    check_closed_form(res, where, theta, n_smpl)
    # the other records are not all of that kind: from a few samples up, variants are called among them
    others = np.setdiff1d(np.arange(cin.n_sites), where)
    assert n_smpl < 3 or (res[2].site["als_new"][others] != 1).any()


def test_twin_ploidy_max_rule(tmp_path):
    """ploidy_max of the definitions behind --ploidy (vcfcall.c:138-199) and of the cases tests/test_c_host_prior.py runs."""
    def pm(text):
        f = tmp_path / "p.txt"
        f.write_text(text)
        return D.ploidy_max(D.parse_ploidy_file(str(f)))
    assert D.ploidy_max(None) == 2
    assert pm("* * * * 1\n") == 1
    assert pm("* * * M 1\n* * * F 2\n") == 2 and pm("* * * M 1\n* * * F 0\n") == 2          # X, Y: no sex '*', the default stays 2
    assert pm("X 1 60000 M 1\nY 1 59373566 F 0\n* * * M 2\n* * * F 2\n") == 2                # GRCh37-like
    assert pm("* * * M 1\n* * * F 1\n") == 2
    assert pm("* * * * 1\nX 1 100 M 2\n") == 2
    assert pm("* * * * 1\nX 1 100 M 1\n") == 1
    assert pm("* * * * 3\n") == 3
