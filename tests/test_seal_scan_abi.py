"""bppp_rp_seal*, bppp_rp_scan* (sealed outputs: a one-sided receive and the view-key scan) are declared in include/bppp.h, admitted by the export
map and exported by the product library, typed in capi.py and wrapped by both handle classes; the status values of the header equal capi's and
rangeproof's; SEAL_BYTES is 34 + 64 nranges everywhere; the two test hooks of the fixed-scalar walk are declared and typed; calls on a NULL
handle fail with BPPP_ERR_ARG without a GPU."""
import fnmatch
import os
import re
import subprocess

from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NARGS = {"bppp_rp_seal": 9, "bppp_rp_seal_device": 9, "bppp_rp_scan": 10, "bppp_rp_scan_device": 10}
HOOKS = {"bppp_test_rp_scan_mul": 5, "bppp_test_rp_scan_recode": 2}


def _header(name="bppp.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_four_symbols_are_declared_exported_and_bound():
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
        for method in ("seal", "scan"):
            assert callable(getattr(cls, method)) and callable(getattr(cls, method + "_device")), method
    assert callable(RP.seal_host) and callable(RP.scan_host)
    assert "rpseal.hip" in open(os.path.join(ROOT, "bulletproofspp_amd", "_build.py")).read()


def test_status_values_and_seal_bytes():
    hdr = _header()
    for name, value in (("SEAL_OK", 0), ("SEAL_NOT_CANONICAL", 1), ("SEAL_ZERO", 2), ("SCAN_FOREIGN", 0), ("SCAN_OWNED", 1), ("SCAN_BAD_HINT", 2), ("SCAN_TAG_ONLY", 3)):
        assert re.search(r"#define\s+BPPP_RP_%s\s+%du?\b" % (name, value), hdr), name
        assert getattr(capi, "RP_" + name) == value and getattr(RP, name) == value, name
    assert re.search(r"#define\s+BPPP_RP_EXCESS_BAD_KEY\s+6u?\b", hdr) and capi.RP_EXCESS_BAD_KEY == RP.EXCESS_BAD_KEY == 6
    macro = re.search(r"#define\s+BPPP_RP_SEAL_BYTES\s*\(\s*(\w+)\s*\)\s*\((.*)\)\s*$", hdr, flags=re.M)
    assert macro
    body = re.sub(r"\(\s*size_t\s*\)", "", macro.group(2))
    for nr in (1, 2, 3, 9, 64):
        assert eval(body, {macro.group(1): nr}) == 34 + 64 * nr == capi.SEAL_BYTES(nr) == RP.SEAL_BYTES(nr)


def test_the_walk_hooks_are_declared_and_typed():
    thdr, tl = _header("bppp_test.h"), capi.load_test_library()
    for name, nargs in HOOKS.items():
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, thdr)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert len(getattr(tl, name).argtypes) == nargs, name


def test_null_handle_is_an_argument_error():
    lib = capi.load_library()
    for n in (0, 1):
        assert lib.bppp_rp_seal(None, n, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_seal_device(None, n, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_scan(None, None, n, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_scan_device(None, None, n, None, None, None, None, None, None, None) == ERR_ARG
    tl = capi.load_test_library()
    assert tl.bppp_test_rp_scan_mul(None, 1, None, None, None) == ERR_ARG and tl.bppp_test_rp_scan_recode(None, None) == ERR_ARG
