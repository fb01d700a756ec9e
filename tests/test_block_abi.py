"""bppp_rp_verify_block / bppp_rp_verify_block_device (a block in one call) are declared in include/bppp.h, admitted by csrc/exports.map, exported by the
built library and typed in capi.py; the two ctypes structs have the sizes and field offsets a C compiler gives the header's; block_seeds is SHA-256
over the 43 bytes the header states; without a GPU, calls on a NULL handle fail with BPPP_ERR_ARG instead of crashing."""
import ctypes as C
import fnmatch
import hashlib
import os
import re
import subprocess

import pytest

from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NAMES = ["bppp_rp_verify_block", "bppp_rp_verify_block_device"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bppp.h")).read(), flags=re.S)


def test_entry_points_are_declared_exported_and_bound():
    lib, hdr = capi.load_library(), _header()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "bulletproofspp_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    dyn = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in dyn.splitlines() if l.strip()}
    for name in NAMES:
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == 6, name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name
        assert name in exported, name
        assert name in capi.SYMBOLS and len(getattr(lib, name).argtypes) == 6, name
    assert "rpblock.hip" in open(os.path.join(ROOT, "bulletproofspp_amd", "_build.py")).read()
    tl = capi.load_test_library()
    assert len(tl.bppp_test_rp_last_block_counts.argtypes) == 5
    assert re.search(r"\bbppp_test_rp_last_block_counts\s*\(", open(os.path.join(ROOT, "include", "bppp_test.h")).read())


def test_structs_match_the_header(tmp_path):
    fields = [(cls, [f for f, _ in cls._fields_]) for cls in (capi.RpBlock, capi.RpBlockStatus)]
    prints = "".join('printf("%%zu", sizeof(%s));' % ("bppp_" + _c_name(cls)) + "".join('printf(" %%zu", offsetof(%s, %s));' % ("bppp_" + _c_name(cls), f) for f in fs) +
                     'printf("\\n");' for cls, fs in fields)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bppp.h"\nint main(void) { %s return 0; }\n' % prints)
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    for (cls, fs), line in zip(fields, lines):
        assert [int(v) for v in line.split()] == [C.sizeof(cls)] + [getattr(cls, f).offset for f in fs], cls.__name__
    hdr = _header()
    body = re.search(r"typedef struct bppp_rp_block \{(.*?)\} bppp_rp_block;", hdr, flags=re.S).group(1)
    assert [n for n in re.findall(r"\*?(\w+)\s*[,;]", body)] == [f for f, _ in capi.RpBlock._fields_]      # the same fields in the same order


def _c_name(cls):
    return {"RpBlock": "rp_block", "RpBlockStatus": "rp_block_status"}[cls.__name__]


def test_block_seeds():
    seed = hashlib.sha256(b"a block seed").digest()
    got = RP.block_seeds(seed)
    assert len(got) == 3 and len(set(got)) == 3
    for p in range(3):
        msg = b"bppp block" + seed + bytes([p])
        assert len(msg) == 43 and got[p] == hashlib.sha256(msg).digest()
    with pytest.raises(ValueError):
        RP.block_seeds(b"short")
    for needle in ('SHA-256 ("bppp block"', "43 bytes", "combined = V + K + S", "shard it"):
        assert needle in open(os.path.join(ROOT, "include", "bppp.h")).read(), needle


def test_null_arguments_are_argument_errors():
    lib = capi.load_library()
    blk, acc = capi.RpBlock(), C.c_int(7)
    for fn in (lib.bppp_rp_verify_block, lib.bppp_rp_verify_block_device):
        assert fn(None, C.byref(blk), None, C.byref(acc), None, None) == ERR_ARG
        assert fn(None, None, None, None, None, None) == ERR_ARG
    assert acc.value == 7
