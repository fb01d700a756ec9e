"""bppp_rp_scan_keys{,_device} (the view-key scan under many secrets in one call) are declared in include/bppp.h with the right argument counts,
admitted by the export map and exported by the product library, typed in capi.py and wrapped by both handle classes; the three test hooks of the
multi-key walk are declared and typed; SCAN_MAX_KEYS equals the header's value everywhere; calls on a NULL handle fail with BPPP_ERR_ARG without
a GPU."""
import fnmatch
import os
import re
import subprocess

from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NARGS = {"bppp_rp_scan_keys": 15, "bppp_rp_scan_keys_device": 15}
HOOKS = {"bppp_test_rp_scan_keys_mul": 6, "bppp_test_rp_scan_keys_recode": 2, "bppp_test_rp_scan_keys_geometry": 4}


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
        assert callable(getattr(cls, "scan_keys")) and callable(getattr(cls, "scan_keys_device"))
    assert callable(RP.scan_keys_host)
    assert "rpscan_keys.hip" in open(os.path.join(ROOT, "bulletproofspp_amd", "_build.py")).read()


def test_max_keys_is_the_headers():
    macro = re.search(r"#define\s+BPPP_RP_SCAN_MAX_KEYS\s+\(\s*\(\s*size_t\s*\)\s*1\s*<<\s*(\d+)\s*\)", _header())
    assert macro and 1 << int(macro.group(1)) == 2**20 == capi.RP_SCAN_MAX_KEYS == RP.SCAN_MAX_KEYS


def test_the_hooks_are_declared_and_typed():
    thdr, tl = _header("bppp_test.h"), capi.load_test_library()
    for name, nargs in HOOKS.items():
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, thdr)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert len(getattr(tl, name).argtypes) == nargs, name


def test_null_handle_is_an_argument_error():
    lib, tl = capi.load_library(), capi.load_test_library()
    for n in (0, 1):
        assert lib.bppp_rp_scan_keys(None, n, None, n, None, None, None, n, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_scan_keys_device(None, n, None, n, None, None, None, n, None, None, None, None, None, None, None) == ERR_ARG
    assert tl.bppp_test_rp_scan_keys_mul(None, 1, None, 1, None, None) == ERR_ARG
    assert tl.bppp_test_rp_scan_keys_recode(None, None) == ERR_ARG and tl.bppp_test_rp_scan_keys_geometry(None, 1, 1, None) == ERR_ARG
