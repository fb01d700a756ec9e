"""examples/c_client/rp_excess.c: a seeded 64bit-shaped handle in plain C99 commits two inputs and two outputs, takes the claim of
inputs - outputs from bppp_rp_tally_claims, signs with its blinding (bppp_rp_excess_sign), sees bppp_rp_excess_verify_each report OK and
bppp_rp_excess_verify_batch accept without being shown the blinding, and sees the same signature refused under another message and with one
output off by one."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_client_excess(tmp_path, gpu):
    lib = os.path.join(ROOT, "bulletproofspp_amd", "lib")
    exe = str(tmp_path / "rp_excess")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_client", "rp_excess.c"),
                    "-L", lib, "-lbppp_hip", "-Wl,-rpath," + lib, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for line in ("claim: amount 500 = the fee", "excess_verify_each: OK", "excess_verify_batch: accept", "another message: MISMATCH, reject",
                 "an output off by one: MISMATCH, reject", "excess c client ok"):
        assert line in p.stdout, (line, p.stdout[-2000:])
