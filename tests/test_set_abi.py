"""The set commitments (bppp_rp_set_*) are declared in include/bppp.h with the right argument counts, admitted by the export map, exported by the
product library, typed in capi.py and wrapped in rangeproof.py; the verdicts and the row limit equal the header's; bppp_rp_set_path_bytes is pure host
code; argument errors need no GPU, and without one no handle, hence no set, can be made."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import pytest

import bulletproofspp_amd as b
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NARGS = {"bppp_rp_set_create": 4, "bppp_rp_set_restore": 5, "bppp_rp_set_destroy": 1, "bppp_rp_set_append": 3, "bppp_rp_set_info": 5, "bppp_rp_set_root": 2,
         "bppp_rp_set_peaks": 2, "bppp_rp_set_path_bytes": 1, "bppp_rp_set_paths": 4, "bppp_rp_set_verify_paths": 10}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bppp.h")).read(), flags=re.S)


def test_the_symbols_are_declared_mapped_exported_and_typed():
    lib, hdr = capi.load_library(), _header()
    dyn = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in dyn.splitlines() if l.strip()}
    emap = open(os.path.join(ROOT, "bulletproofspp_amd", "csrc", "exports.map")).read()
    patterns = re.search(r"global:\s*([^;]*);", emap).group(1).split()
    for name, nargs in NARGS.items():
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert not re.search(r"\bd_\w+", decl.group(1)), name + ": every buffer is on the host"
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name
        assert name in exported, name
        assert name in capi.SYMBOLS and len(getattr(lib, name).argtypes) == nargs, name
    assert lib.bppp_rp_set_destroy.restype is None and lib.bppp_rp_set_path_bytes.restype is C.c_size_t
    for name in ("append", "root", "peaks", "paths", "info", "restore", "close"):
        assert callable(getattr(RP.CommitmentSet, name)), name
    for name in ("commitment_set", "set_verify_paths", "set_path_bytes"):
        assert callable(getattr(RP.NativeRangeProofs, name)), name
    for name in ("set_leaf_host", "set_peaks_host", "set_root_host", "set_path_host", "set_verify_path_host", "set_path_bytes"):
        assert callable(getattr(RP, name)), name
    assert "rpset.hip" in open(os.path.join(ROOT, "bulletproofspp_amd", "_build.py")).read()


def test_the_verdicts_and_the_limit_are_the_headers():
    hdr = _header()
    val = lambda name: int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, hdr).group(1))
    assert (val("BPPP_RP_SET_OK"), val("BPPP_RP_SET_MISMATCH"), val("BPPP_RP_SET_BAD_INDEX"), val("BPPP_RP_SET_BAD_PADDING")) == (0, 1, 2, 3)
    assert (capi.RP_SET_OK, capi.RP_SET_MISMATCH, capi.RP_SET_BAD_INDEX, capi.RP_SET_BAD_PADDING) == (0, 1, 2, 3)
    assert (RP.SET_OK, RP.SET_MISMATCH, RP.SET_BAD_INDEX, RP.SET_BAD_PADDING) == (0, 1, 2, 3)
    assert val("BPPP_RP_SET_MAX_ROW_BYTES") == 8192 == capi.RP_SET_MAX_ROW_BYTES == RP.SET_MAX_ROW_BYTES
    plan = open(os.path.join(ROOT, "bulletproofspp_amd", "csrc", "rpset_plan.hpp")).read()
    assert re.search(r"MAX_ROW_BYTES\s*=\s*8192\b", plan)


def test_path_bytes_is_host_code():
    lib = capi.load_library()
    for n in [0, 1, 2, 3, 4, 255, 256, 2**31 - 1, 2**31, 2**62, 2**63 - 1, 2**64 - 1]:
        assert lib.bppp_rp_set_path_bytes(n) == 32 * n.bit_length() == RP.set_path_bytes(n) == RP.NativeRangeProofs.set_path_bytes(n)


def test_argument_errors_need_no_gpu():
    lib = capi.load_library()
    out, acc = C.c_void_p(0x1234), C.c_int(7)
    assert lib.bppp_rp_set_create(None, 33, 1, C.byref(out)) == ERR_ARG and lib.bppp_rp_set_create(None, 33, 1, None) == ERR_ARG
    assert lib.bppp_rp_set_restore(None, 33, 0, None, C.byref(out)) == ERR_ARG
    assert lib.bppp_rp_set_append(None, 0, None) == ERR_ARG and lib.bppp_rp_set_append(None, 1, None) == ERR_ARG
    assert lib.bppp_rp_set_info(None, None, None, None, None) == ERR_ARG
    assert lib.bppp_rp_set_root(None, None) == ERR_ARG and lib.bppp_rp_set_peaks(None, None) == ERR_ARG
    assert lib.bppp_rp_set_paths(None, 0, None, None) == ERR_ARG
    assert lib.bppp_rp_set_verify_paths(None, 33, 1, None, 0, None, None, None, None, C.byref(acc)) == ERR_ARG and acc.value == 7
    assert lib.bppp_rp_set_verify_paths(None, 33, 1, None, 0, None, None, None, None, None) == ERR_ARG
    lib.bppp_rp_set_destroy(None)


def test_without_a_gpu_create_fails_loudly():
    """a set lives on a range-proof handle, a handle on a context: where no GPU is the context cannot be made (BpppError), and a set asked of no handle
    is an argument error that leaves the out pointer NULL"""
    import torch
    lib = capi.load_library()
    out = C.c_void_p(0x1234)
    assert lib.bppp_rp_set_create(None, 33, 0, C.byref(out)) == ERR_ARG and not out.value
    if not torch.cuda.is_available():
        with pytest.raises(b.BpppError):
            b.Bppp(0)
