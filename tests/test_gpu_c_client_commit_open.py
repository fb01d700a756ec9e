"""examples/c_client/rp_commit_open.c: a seeded handle in plain C99 commits two rows (bppp_rp_commit_batch), opens them (bppp_rp_open_each,
bppp_rp_open_batch), sees BPPP_RP_OPEN_MISMATCH for an amount that is off by one, and finds the prover's commitments files equal to its own."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_client_commit_open(tmp_path, gpu):
    lib = os.path.join(ROOT, "bulletproofspp_amd", "lib")
    exe = str(tmp_path / "rp_commit_open")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_client", "rp_commit_open.c"),
                    "-L", lib, "-lbppp_hip", "-Wl,-rpath," + lib, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "commit / open c client ok" in p.stdout, (p.stdout[-2000:], p.stderr[-2000:])
