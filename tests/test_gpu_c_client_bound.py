"""examples/c_client/rp_bound.c: a seeded handle in plain C99 proves two transactions under two bindings (bppp_rp_prove_bound), sees them accepted
with their own bindings (bppp_rp_verify_bound), and refused with the two bindings swapped and without any."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_client_bound(tmp_path, gpu):
    lib = os.path.join(ROOT, "bulletproofspp_amd", "lib")
    exe = str(tmp_path / "rp_bound")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_client", "rp_bound.c"),
                    "-L", lib, "-lbppp_hip", "-Wl,-rpath," + lib, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    out = p.stdout
    assert "own bindings:     accept 1, statuses 0 0" in out, out
    assert "swapped bindings: accept 0, statuses 1 1" in out, out
    assert "no bindings:      accept 0, statuses 1 1" in out, out
    assert "bound c client ok" in out, out
