"""The per-proof public-amount entry points (bppp_rp_*_pub, bppp_rp_public_count) are declared in include/bppp.h, exported by the product
library and typed in capi.py; without a GPU, calls on a NULL handle fail with BPPP_ERR_ARG instead of crashing."""
import ctypes as C
import os
import re

from bulletproofspp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bppp_rp_public_count", "bppp_rp_verify_batch_pub", "bppp_rp_verify_batch_pub_device", "bppp_rp_verify_shard_pub_device",
       "bppp_rp_verify_each_pub", "bppp_rp_verify_each_pub_device", "bppp_rp_prove_batch_pub"]


def test_public_amount_entry_points_are_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bppp.h")).read(), flags=re.S)
    lib = capi.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name


def test_public_amount_entry_points_refuse_a_null_handle():
    lib = capi.load_library()
    n = C.c_size_t(5)
    acc = C.c_int(0)
    assert lib.bppp_rp_public_count(None, C.byref(n)) == -1 and n.value == 5
    assert lib.bppp_rp_verify_batch_pub(None, 1, None, None, None, None, C.byref(acc), None, None, None) == -1
    assert lib.bppp_rp_verify_shard_pub_device(None, 1, 0, None, None, None, None, C.byref(acc), None, None, None) == -1
    assert lib.bppp_rp_verify_each_pub(None, 1, None, None, None, None, None) == -1
    assert lib.bppp_rp_prove_batch_pub(None, 1, None, None, None, None, None, 0, None, None) == -1
