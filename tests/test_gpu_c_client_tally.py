"""examples/c_client/rp_tally.c: a seeded 64bit-shaped handle in plain C99 commits two inputs and two outputs, takes the claim of
inputs - outputs from bppp_rp_tally_claims (its amount is the fee), sees bppp_rp_tally_each report OK and bppp_rp_tally_batch accept, and with one
output off by one sees MISMATCH and a rejection."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_client_tally(tmp_path, gpu):
    lib = os.path.join(ROOT, "bulletproofspp_amd", "lib")
    exe = str(tmp_path / "rp_tally")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_client", "rp_tally.c"),
                    "-L", lib, "-lbppp_hip", "-Wl,-rpath," + lib, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for line in ("claim: amount 500 = the fee", "tally_each: OK", "tally_batch: accept", "tally_each, an output off by one: MISMATCH",
                 "tally_batch, an output off by one: reject", "tally c client ok"):
        assert line in p.stdout, (line, p.stdout[-2000:])
