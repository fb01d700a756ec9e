"""examples/c_client/rp_cut_through.c: a seeded 64bit-shaped handle in plain C99 builds two transactions (A into B and C, then B into D), states
each excess as a 33-byte key (bppp_rp_excess_keys) signed by bppp_rp_excess_sign, and checks the block after cut-through — only - A + C + D, the
summed fee and the summed offset are left: bppp_rp_excess_verify_keys_batch accepts the signatures with no commitment in hand,
bppp_rp_excess_sums_each reports OK and bppp_rp_excess_sums_batch accepts; a key left out, a fee off by one and a signature under the other
transaction's key are each MISMATCH."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_client_cut_through(tmp_path, gpu):
    lib = os.path.join(ROOT, "bulletproofspp_amd", "lib")
    exe = str(tmp_path / "rp_cut_through")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_client", "rp_cut_through.c"),
                    "-L", lib, "-lbppp_hip", "-Wl,-rpath," + lib, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for line in ("builders: two keys of 33 bytes", "verify_keys_batch: accept", "sums_each: OK with B cut through", "sums_batch: accept", "one key left out: MISMATCH",
                 "a fee off by one: MISMATCH, reject", "a signature under the other key: MISMATCH, reject", "cut-through c client ok"):
        assert line in p.stdout, (line, p.stdout[-2000:])
