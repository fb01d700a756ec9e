"""bppp_rp_commit_batch*, bppp_rp_open_each* and bppp_rp_open_batch* (commitments without a proof, and checking their openings) are declared in
include/bppp.h, exported by the product library, covered by csrc/exports.map and typed in capi.py; the status values are the header's; the
weight message of bppp_rp_open_batch, as rangeproof.open_weight restates it, is pinned against one vector put together by hand; without a GPU,
calls on a NULL handle fail with BPPP_ERR_ARG instead of crashing."""
import fnmatch
import hashlib
import os
import re
import subprocess

from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NAMES = ["bppp_rp_commit_batch", "bppp_rp_commit_batch_device", "bppp_rp_open_each", "bppp_rp_open_each_device", "bppp_rp_open_batch",
         "bppp_rp_open_batch_device"]
NARGS = {"bppp_rp_commit_batch": 7, "bppp_rp_commit_batch_device": 7, "bppp_rp_open_each": 7, "bppp_rp_open_each_device": 7, "bppp_rp_open_batch": 10,
         "bppp_rp_open_batch_device": 11}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bppp.h")).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(bppp_\w+)\s*\(", _header())))


def test_entry_points_are_declared_exported_and_bound():
    lib, hdr = capi.load_library(), _header()
    dyn = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in dyn.splitlines() if l.strip()}
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in exported, name
        assert name in capi.SYMBOLS and len(getattr(lib, name).argtypes) == NARGS[name], name
    from bulletproofspp_amd.rangeproof_binary import NativeBinaryRangeProofs
    for cls in (RP.NativeRangeProofs, NativeBinaryRangeProofs):
        for method in ("commit_batch", "commit_batch_device", "open_each", "open_each_device", "open_batch", "open_batch_device"):
            assert callable(getattr(cls, method)), method


def test_exports_map_equals_the_header():
    """the version script's global patterns admit every declared symbol, the dynamic symbol table holds exactly the declared ones"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "bulletproofspp_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    declared = _declared()
    assert patterns and all(any(fnmatch.fnmatchcase(n, p) for p in patterns) for n in declared)
    dyn = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[-1] for l in dyn.splitlines() if l.strip()) == declared


def test_status_values():
    hdr = _header()
    want = {"BPPP_RP_COMMIT_INFINITY": 16, "BPPP_RP_OPEN_OK": 0, "BPPP_RP_OPEN_MISMATCH": 1, "BPPP_RP_OPEN_MALFORMED": 2, "BPPP_RP_OPEN_NOT_CANONICAL": 3}
    for name, value in want.items():
        assert re.search(r"#define\s+%s\s+%du\b" % (name, value), hdr), name
        assert getattr(capi, name[len("BPPP_"):]) == value
    assert capi.RP_COMMIT_INFINITY not in (capi.RP_WIT_OK, capi.RP_WIT_NOT_CANONICAL, capi.RP_WIT_UNBALANCED, capi.RP_WIT_OUT_OF_RANGE, capi.RP_WIT_BIN_NOT_CANONICAL,
                                           capi.RP_WIT_BIN_UNBALANCED)


def test_open_weight_vector():
    """seed || le64(j) || x || sign || put(v) || put(ty) || put(bl), put = four 64-bit limbs least significant first, each big-endian; the
    digest read the same way and reduced mod n"""
    seed = bytes(range(32))
    j, sign = 0x0102030405060708, 1
    x = bytes(range(100, 132))
    v, ty, bl = 5, 2**64 + 7, RP.N - 1
    msg = seed + bytes([8, 7, 6, 5, 4, 3, 2, 1]) + x + b"\x01"
    msg += (5).to_bytes(8, "big") + bytes(24)                                         # v: limb 0 = 5
    msg += (7).to_bytes(8, "big") + (1).to_bytes(8, "big") + bytes(16)                # ty: limb 0 = 7, limb 1 = 1
    nm1 = RP.N - 1
    msg += b"".join(((nm1 >> (64 * i)) & (2**64 - 1)).to_bytes(8, "big") for i in range(4))
    assert len(msg) == 169
    d = hashlib.sha256(msg).digest()
    want = sum(int.from_bytes(d[8 * i:8 * i + 8], "big") << (64 * i) for i in range(4)) % RP.N
    assert want != 0 and RP.open_weight(seed, j, x, sign, v, ty, bl) == want
    assert RP.open_weight(seed, j + 1, x, sign, v, ty, bl) != want and RP.open_weight(seed, j, x, 0, v, ty, bl) != want


def test_null_handle_is_an_argument_error():
    lib = capi.load_library()
    for batch in (0, 1):
        assert lib.bppp_rp_commit_batch(None, batch, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_commit_batch_device(None, batch, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_open_each(None, batch, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_open_each_device(None, batch, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_open_batch(None, batch, None, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_open_batch_device(None, batch, 0, None, None, None, None, None, None, None, None) == ERR_ARG
