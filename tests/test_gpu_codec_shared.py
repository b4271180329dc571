"""The four encoder entries share one scan buffer and one pinned total (enc_offsets: WS_COMPACT_ENC_SCAN_TMP, PIN_ENC_TOTAL).  On one
context bcfgpu_mplp_encode_bcf, bcfgpu_mplp_encode_vcf, bcfgpu_call_encode_bcf, bcfgpu_call_remap_bcf and bcfgpu_call_decode_bcf are
called one after the other, in one order and in the reverse one, with a call that returns E_RANGE (a buffer one byte short) and a
call with nothing to encode among them: every result is its twin's (tests/helpers), byte for byte and offset for offset.  The inputs
are those of the entries' own tests, cut to a few sites: 3 and 65 samples (one and two wavefronts; blocks below a 16-byte line and of
many lines), scans of n + 1, 3 n + 1 and n_keys + 1 sizes with three different lengths."""
import numpy as np
import pytest

from bcftools_amd import abi, engine
from tests import test_gpu_call_bcf_encode as call_case, test_gpu_call_key_encode as key_case, test_gpu_vcf_encode as mplp_case
from tests.helpers import bcfdec, bcfenc, callenc, keyenc, vcfenc

pytestmark = pytest.mark.gpu

ALL_FMT = mplp_case.ALL_FMT
IDS = {k: 5 + i for i, k in enumerate(abi.BCF_KEYS)}
CALL_IDS = call_case.IDS
N_MPLP, N_CALL, N_REC, N_PLANES = 7, 5, 2, 5                    # scans of 8, 16 and 7 sizes (three jobs a record)


def starts(off):
    """The start offsets mod 16 of the blocks that are not empty."""
    return {int(x) % 16 for x in off[:-1][np.diff(off.astype(np.int64)) > 0]}


def check_equal(got, exp):
    data, off = got
    wdata, woff = exp
    assert len(off) == len(woff)
    np.testing.assert_array_equal(off, woff)
    assert data.tobytes() == wdata.tobytes()


@pytest.mark.parametrize("S", [3, 65])
def test_the_entries_in_turn_on_one_context(S):
    rng = np.random.default_rng(S)
    mplp = mplp_case.mixed_planes(rng, N_MPLP, S)
    call = call_case.planes(rng, N_CALL, S)
    call.pl[1, 0, S // 2], call.pl[3, 0, 0] = 40000, 99999       # an int16 and an int32 PL among the int8 ones
    indiv, keys, site = key_case.jobs(S, n=N_REC)
    vec = [(int(k["off"]), int(k["type"]), int(k["width"])) for k in keys]

    want_bcf = bcfenc.encode_planes(ALL_FMT, IDS, mplp.site["n_alleles"], mplp.pl, mplp.dp4, mplp.adf, mplp.adr, mplp.qs, mplp.scr, mplp.sp)
    want_vcf = mplp_case.want(ALL_FMT, mplp)
    want_call = callenc.encode_planes(CALL_IDS, call.site, call.gt, call.pl, call.gq)
    want_keys = keyenc.encode_jobs(indiv, keys, S, site, S)
    want_dec = bcfdec.decode_vec(indiv, vec, S, N_PLANES)
    assert len({len(w[1]) for w in (want_bcf, want_call, want_keys)}) == 3 and len(want_vcf[1]) == N_MPLP + 1
    for w in (want_bcf, want_vcf, want_call, want_keys):
        assert len(starts(w[1])) >= 4                           # the blocks start at several bytes of a 16-byte line
    sizes = np.concatenate([np.diff(w[1].astype(np.int64)) for w in (want_bcf, want_vcf, want_call, want_keys)])
    assert (sizes[sizes > 0] < 16).any() == (S == 3) and (sizes > 256).any()      # blocks below a line (3 samples) and of many lines

    with engine.Context(abi.default_cfg(S, max_sites=8, max_reads=64, fmt_flag=ALL_FMT)) as ctx:
        d_mplp, d_call = mplp_case.upload(ctx, mplp), call_case.upload(ctx, call)

        def short(encode, need):
            """The entry with a buffer one byte short: E_RANGE and the size it needs."""
            with pytest.raises(engine.BcfGpuError) as e:
                encode(need - 1)
            assert e.value.code == abi.E_RANGE and e.value.needed == need

        def nothing(got):
            assert len(got[0]) == 0 and got[1].tolist() == [0]

        steps = [
            lambda: check_equal(ctx.encode_bcf(d_mplp, N_MPLP, IDS), want_bcf),
            lambda: short(lambda cap: ctx.encode_vcf(d_mplp, N_MPLP, cap_bytes=cap), len(want_vcf[0])),
            lambda: check_equal(ctx.encode_call_bcf(d_call, N_CALL, abi.MAX_PL, CALL_IDS), want_call),
            lambda: nothing(ctx.encode_bcf(d_mplp, 0, IDS)),
            lambda: check_equal(ctx.remap_call_bcf(indiv, keys, S, site), want_keys),
            lambda: short(lambda cap: ctx.encode_call_bcf(d_call, N_CALL, abi.MAX_PL, CALL_IDS, cap_bytes=cap), len(want_call[0])),
            lambda: check_equal(ctx.encode_vcf(d_mplp, N_MPLP), want_vcf),
            lambda: nothing(ctx.remap_call_bcf(indiv, keys[:0], S, site)),
            lambda: np.testing.assert_array_equal(ctx.decode_bcf(indiv, vec, S, N_PLANES), want_dec),
        ]
        for step in steps + steps[::-1]:
            step()
