"""The six bppp_rp_*_bound* entry points (per-proof transcript bindings) are declared in include/bppp.h, admitted by csrc/exports.map, exported by
the built library and typed in capi.py; BPPP_RP_BINDING_BYTES is 32; the Python wrappers refuse a binding of the wrong size with ValueError
before any library call; without a GPU, calls on a NULL handle fail with BPPP_ERR_ARG instead of crashing."""
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd.rangeproof_binary import NativeBinaryRangeProofs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NARGS = {"bppp_rp_verify_bound": 11, "bppp_rp_verify_bound_device": 12, "bppp_rp_verify_each_bound": 8, "bppp_rp_verify_each_bound_device": 8,
         "bppp_rp_prove_bound": 12, "bppp_rp_prove_bound_device": 12}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bppp.h")).read(), flags=re.S)


def test_entry_points_are_declared_exported_and_bound():
    lib, hdr = capi.load_library(), _header()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "bulletproofspp_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    dyn = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in dyn.splitlines() if l.strip()}
    for name, nargs in NARGS.items():
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name
        assert name in exported, name
        assert name in capi.SYMBOLS and len(getattr(lib, name).argtypes) == nargs, name


def test_binding_size():
    assert re.search(r"#define\s+BPPP_RP_BINDING_BYTES\s+32\b", _header())
    assert capi.RP_BINDING_BYTES == 32


def test_the_header_states_the_tag_limit_and_what_is_not_covered():
    raw = open(os.path.join(ROOT, "include", "bppp.h")).read()
    sect = raw[raw.index("per-proof transcript bindings"):raw.index("#define BPPP_RP_BINDING_BYTES")]
    for needle in ("app/Main.hs:75-80", "src/ZKP.hs:96-101", "Tag limit", "bppp_rp_verify_mixed", "bppp_rp_prove_mixed", "commit / open"):
        assert needle in sect, needle


def test_bindings_array():
    good = [bytes(range(32)), b"\xff" * 32, bytes(32)]
    arr = capi.bindings_array(good, 3)
    assert arr.dtype == np.uint8 and arr.shape == (3, 32) and arr.flags["C_CONTIGUOUS"] and arr.tobytes() == b"".join(good)
    assert capi.bindings_array(arr, 3).tobytes() == arr.tobytes()
    assert capi.bindings_array(None, 3) is None
    for bad in ([bytes(31)] + good[1:], good[:2], np.zeros((3, 33), dtype=np.uint8), np.zeros((2, 32), dtype=np.uint8), np.zeros((3, 32), dtype=np.uint32),
                [b"x" * 32, "y" * 32, b"z" * 32]):
        with pytest.raises(ValueError):
            capi.bindings_array(bad, 3)


class _NoLibrary:
    """stands where a wrapper keeps its Bppp handle: any use of it is a library call made before the bindings were checked"""

    def __getattr__(self, name):
        raise AssertionError("the wrapper reached the library (%s) before it checked the bindings" % name)


@pytest.mark.parametrize("cls", [RP.NativeRangeProofs, NativeBinaryRangeProofs])
def test_wrappers_reject_a_bad_binding_before_any_call(cls):
    nat = cls.__new__(cls)                          # no handle, no GPU: only the argument checks can run
    nat.gpu, nat.h, nat.st = _NoLibrary(), None, None
    nat.shape = {"coms_bytes": 4, "proof_bytes": 4, "challenges_per_proof": 1, "rounds": 0}
    short = [bytes(31)] * 2
    wide = np.zeros((2, 33), dtype=np.uint8)
    files = [b"abcd", b"efgh"]
    for bad in (short, wide):
        with pytest.raises(ValueError):
            nat.prove_batch([[], []], [b"p", b"q"], bindings=bad)
        with pytest.raises(ValueError):
            nat.prove_batch_status([[], []], [b"p", b"q"], bindings=bad)
        with pytest.raises(ValueError):
            nat.prove_batch_device(2, 16, 16, 16, 16, 1, 16, 16, bindings=bad)
        with pytest.raises(ValueError):
            nat.prove_batch_status_device(2, 16, 16, 16, 16, 1, 16, 16, bindings=bad)
        with pytest.raises(ValueError):
            nat.verify_batch(files, files, b"s" * 32, bindings=bad)
        with pytest.raises(ValueError):
            nat.verify_batch_device(2, 16, 16, b"s" * 32, bindings=bad)
        with pytest.raises(ValueError):
            nat.verify_each(files, files, bindings=bad)
        with pytest.raises(ValueError):
            nat.verify_each_device(2, 16, 16, bindings=bad)
    nat.h = None                                    # (__del__ must find nothing to destroy)


def test_null_handle_is_an_argument_error():
    lib = capi.load_library()
    for batch in (0, 1):
        assert lib.bppp_rp_verify_bound(None, batch, None, None, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_verify_bound_device(None, batch, 0, None, None, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_verify_each_bound(None, batch, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_verify_each_bound_device(None, batch, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_prove_bound(None, batch, None, None, None, None, None, None, 0, None, None, None) == ERR_ARG
        assert lib.bppp_rp_prove_bound_device(None, batch, None, None, None, None, None, None, 0, None, None, None) == ERR_ARG
