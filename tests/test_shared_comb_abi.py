"""Shared comb tables and the mixed-setup prover at the ABI level (no GPU): bppp_rp_share_comb, bppp_rp_comb_info and bppp_rp_prove_mixed
are declared in include/bppp.h, exported by the gfx950 library the build cross-compiles, and bound by capi.py with the header's argument
types; the Python layer exposes them."""
import ctypes as C
import os
import re
import subprocess

import pytest

from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bppp_rp_share_comb", "bppp_rp_comb_info", "bppp_rp_prove_mixed"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.lib_path()):
        import __graft_entry__ as g
        g.build()
    return capi.load_library()


def test_declared_once_in_the_header():
    text = open(os.path.join(ROOT, "include", "bppp.h")).read()
    for name in NEW:
        assert len(re.findall(r"^int %s\(" % name, text, flags=re.M)) == 1, name
    assert "typedef struct bppp_rp_prove_group" in text


def test_exported_by_the_built_library(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert name in exported and name in capi.SYMBOLS and hasattr(lib, name), name


def test_bound_with_the_header_argument_types(lib):
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    assert lib.bppp_rp_share_comb.argtypes == [vp, vp]
    assert lib.bppp_rp_comb_info.argtypes == [vp, C.POINTER(i), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    assert lib.bppp_rp_prove_mixed.argtypes == [vp, sz]
    # bppp_rp_prove_group, field by field as the header lays it out
    want = [("rp", vp), ("batch", sz), ("amounts", vp), ("types", vp), ("blinds", vp), ("public_amounts", vp), ("rand_prefix", vp), ("prefix_len", sz),
            ("coms_files", vp), ("proof_files", vp)]
    assert capi.RpProveGroup._fields_ == want
    assert C.sizeof(capi.RpProveGroup) == 10 * 8


def test_null_handles_and_the_empty_job(lib):
    """the argument checks that need no context: a null handle is BPPP_ERR_ARG (-1), an empty job is BPPP_OK"""
    assert lib.bppp_rp_share_comb(None, None) == -1
    assert lib.bppp_rp_comb_info(None, None, None, None, None) == -1
    assert lib.bppp_rp_prove_mixed(None, 0) == 0
    assert lib.bppp_rp_prove_mixed(None, 2) == -1
    groups = (capi.RpProveGroup * 1)()          # one group without a handle
    assert lib.bppp_rp_prove_mixed(C.cast(groups, C.c_void_p), 1) == -1


def test_python_layer():
    assert callable(RP.prove_mixed) and callable(RP.NativeRangeProofs.share_comb) and callable(RP.NativeRangeProofs.comb_info)
