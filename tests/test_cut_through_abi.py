"""bppp_rp_cut_through{,_device} (the transactions of a block merged into its one sum) are declared in include/bppp.h with the right argument counts,
admitted by the export map and exported by the product library, typed in capi.py and wrapped by both handle classes; the verdict codes and the counts
struct agree between the header and capi.py; the two test hooks are declared and typed; the kernels' file is built; calls on a NULL handle fail with
BPPP_ERR_ARG without a GPU."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NARGS = {"bppp_rp_cut_through": 16, "bppp_rp_cut_through_device": 16}
HOOKS = {"bppp_test_rp_cut_through_force": 4, "bppp_test_rp_cut_through_last": 4}


def _header(name="bppp.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_both_symbols_are_declared_exported_and_bound():
    lib, hdr = capi.load_library(), _header()
    dyn = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in dyn.splitlines() if l.strip()}
    emap = open(os.path.join(ROOT, "bulletproofspp_amd", "csrc", "exports.map")).read()
    patterns = re.search(r"global:\s*([^;]*);", emap).group(1).split()
    for name, nargs in NARGS.items():
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name
        assert name in exported, name
        assert name in capi.SYMBOLS and len(getattr(lib, name).argtypes) == nargs, name
    for cls in (RP.NativeRangeProofs, BRP.NativeBinaryRangeProofs):
        for method in ("cut_through", "cut_through_device", "assemble_block"):
            assert callable(getattr(cls, method)), (cls, method)
    assert callable(RP.cut_through_host) and callable(RP.cut_identity)
    build = open(os.path.join(ROOT, "bulletproofspp_amd", "_build.py")).read()
    assert '"rpcut.hip"' in build
    assert os.path.exists(os.path.join(ROOT, "bulletproofspp_amd", "csrc", "rpcut.hip")) and os.path.exists(os.path.join(ROOT, "bulletproofspp_amd", "csrc", "rpcut.hip.h"))


def test_codes_and_counts_are_the_headers():
    hdr = _header()
    for name, value in (("KEPT", 0), ("SPENT", 1), ("KEPT_AGAIN", 2)):
        macro = re.search(r"#define\s+BPPP_RP_CUT_%s\s+(\d+)u" % name, hdr)
        assert macro and int(macro.group(1)) == value == getattr(capi, "RP_CUT_" + name) == getattr(RP, "CUT_" + name), name
    struct = re.search(r"typedef struct bppp_rp_cut_counts\s*\{([^}]*)\}", hdr)
    fields = [f.strip() for f in struct.group(1).replace("size_t", "").replace(";", "").split(",")]
    assert fields == [n for n, _ in capi.RpCutCounts._fields_] == ["new_rows", "out_rows", "new_nnz", "ncut", "nagain"]
    assert all(t is C.c_size_t for _, t in capi.RpCutCounts._fields_)


def test_the_hooks_are_declared_and_typed():
    thdr, tl, lib = _header("bppp_test.h"), capi.load_test_library(), capi.load_library()
    for name, nargs in HOOKS.items():
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, thdr)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert len(getattr(tl, name).argtypes) == nargs, name
        assert not hasattr(lib, name), name


def test_null_handle_is_an_argument_error():
    lib, tl = capi.load_library(), capi.load_test_library()
    cnt = capi.RpCutCounts()
    for n in (0, 1):
        for fn in (lib.bppp_rp_cut_through, lib.bppp_rp_cut_through_device):
            assert fn(None, n, None, n, None, None, n, None, None, None, None, None, None, None, None, C.byref(cnt)) == ERR_ARG
            assert fn(None, n, None, n, None, None, n, None, None, None, None, None, None, None, None, None) == ERR_ARG
    salt = (C.c_uint8 * 16)()
    g = C.c_uint64()
    assert tl.bppp_test_rp_cut_through_force(None, 1, salt, 1) == ERR_ARG
    assert tl.bppp_test_rp_cut_through_last(None, C.byref(g), C.byref(g), C.byref(g)) == ERR_ARG
