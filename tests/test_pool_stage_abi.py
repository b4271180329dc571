"""The staged read pool's boundary without a GPU: include/bcfgpu.h declares bcfgpu_pool_stage and bcfgpu_pool_adopt, the
library exports them, bcftools_amd.abi mirrors them, both refuse a NULL context before they touch a device, and the slots a
staged pool lies in keep the rules of the context's slot table (bcftools_amd/csrc/ctx.h): kept from the stage to the adopt, each
number used by no other name."""
import ctypes as C

from bcftools_amd import abi, lib
from tests.test_abi import declared_functions
from tests.test_ctx_slots import CTX_H, parse_enum, parse_kept, slot_violations

CALLS = ("bcfgpu_pool_stage", "bcfgpu_pool_adopt")
# the pool's slots before a staged pool existed: one set of its arrays, the keep mask
ONE_SET = {"WS_POOL_CIG", "WS_POOL_SEQ16", "WS_POOL_QUAL", "WS_POOL_R_POS", "WS_POOL_R_LQ", "WS_POOL_R_FLAG", "WS_POOL_R_NCIG",
           "WS_POOL_R_CIG_OFF", "WS_POOL_R_SEQ_OFF", "WS_POOL_R_MAPQ", "WS_POOL_KEEP"}


def test_header_library_and_mirror_have_both_calls():
    L = lib.load()
    declared = declared_functions()
    for name in CALLS:
        assert name in declared, "include/bcfgpu.h does not declare %s" % name
        assert hasattr(L, name), "libbcfgpu.so does not export %s" % name
        assert name in abi.PROTOTYPES
    assert abi.PROTOTYPES["bcfgpu_pool_stage"] == abi.PROTOTYPES["bcfgpu_pool_upload"]        # exactly the upload's arguments
    assert abi.PROTOTYPES["bcfgpu_pool_adopt"] == (C.c_int, [C.c_void_p])


def test_null_context_is_refused_without_a_device():
    L = lib.load()
    rd = abi.Reads()
    assert L.bcfgpu_pool_stage(None, C.byref(rd), None, None) == abi.E_ARG
    assert b"bcfgpu_pool_stage" in L.bcfgpu_last_error()
    assert L.bcfgpu_pool_adopt(None) == abi.E_ARG
    assert b"bcfgpu_pool_adopt" in L.bcfgpu_last_error()


def test_staged_pool_slots_are_kept_and_their_own():
    with open(CTX_H) as f:
        text = f.read()
    assert slot_violations(text) == []
    ws = parse_enum(text, "WsSlot")
    ws.pop("WS_COUNT")
    kept = parse_kept(text)
    new = [k for k in kept if k.startswith("WS_POOL_") and k not in ONE_SET]
    # a second set of the ten arrays DevPool points at, and the packed inputs (seq4, qual4, the records) from stage to adopt
    assert len(new) >= 13, new
    for k in new:
        same = [o for o, v in ws.items() if v == ws[k] and o != k]
        assert not same, "%s = %d is also %s" % (k, ws[k], same)
    # the staged records are not the slot bcfgpu_pool_baq sorts its jobs in (it runs on the current pool during a stage)
    assert all(ws[k] != ws["WS_PBAQ_JOBS2_SORTED"] for k in new)
