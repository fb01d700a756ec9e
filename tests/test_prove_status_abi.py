"""bppp_rp_prove_batch_status, bppp_rp_prove_batch_status_device and bppp_rp_witness_status_text (per-proof witness verdicts for the batch prover)
are declared in include/bppp.h, exported by the product library and typed in capi.py; the BPPP_RP_WIT_* values and their texts are the witness
kernels' status words; without a GPU, calls on a NULL handle fail with BPPP_ERR_ARG instead of crashing."""
import os
import re

from bulletproofspp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NAMES = ["bppp_rp_prove_batch_status", "bppp_rp_prove_batch_status_device", "bppp_rp_witness_status_text"]
TEXTS = {1: "type / blinding not canonical", 2: "amounts of some type do not balance", 3: "value outside its range", 4: "blinding is not canonical",
         5: "a binary witness needs a conserved schema whose amounts balance (Binary.hs:162-164)"}


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_status_entry_points_are_declared_exported_and_bound():
    lib, hdr = capi.load_library(), _header("bppp.h")
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert len(lib.bppp_rp_prove_batch_status.argtypes) == 11 and len(lib.bppp_rp_prove_batch_status_device.argtypes) == 11
    assert callable(getattr(capi.Bppp, "rp_prove_batch_status_device"))
    from bulletproofspp_amd.rangeproof import NativeRangeProofs
    from bulletproofspp_amd.rangeproof_binary import NativeBinaryRangeProofs
    for cls in (NativeRangeProofs, NativeBinaryRangeProofs):
        assert callable(cls.prove_batch_status) and callable(cls.prove_batch_status_device)


def test_status_values_and_texts():
    lib, hdr = capi.load_library(), _header("bppp.h")
    want = {"OK": 0, "NOT_CANONICAL": 1, "UNBALANCED": 2, "OUT_OF_RANGE": 3, "BIN_NOT_CANONICAL": 4, "BIN_UNBALANCED": 5}
    for name, value in want.items():
        assert re.search(r"#define\s+BPPP_RP_WIT_%s\s+%du\b" % (name, value), hdr), name
        assert getattr(capi, "RP_WIT_" + name) == value
    for code, text in TEXTS.items():
        assert lib.bppp_rp_witness_status_text(code).decode() == text
    assert lib.bppp_rp_witness_status_text(77) is not None          # any other value: a static string, never NULL


def test_null_handle_is_an_argument_error():
    lib = capi.load_library()
    for batch in (0, 1):
        assert lib.bppp_rp_prove_batch_status(None, batch, None, None, None, None, None, 0, None, None, None) == ERR_ARG
        assert lib.bppp_rp_prove_batch_status_device(None, batch, None, None, None, None, None, 0, None, None, None) == ERR_ARG
