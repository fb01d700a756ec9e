"""examples/c_client/rp_one_sided.c: a seeded handle in plain C99 seals two outputs to a view key (bppp_rp_excess_keys, bppp_rp_seal), proves with
the returned blindings and verifies, then scans four rows (bppp_rp_scan): the two, a foreign one and one with a flipped memo bit, and prints the
verdicts and the recovered amounts."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_client_one_sided(tmp_path, gpu):
    lib = os.path.join(ROOT, "bulletproofspp_amd", "lib")
    exe = str(tmp_path / "rp_one_sided")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_client", "rp_one_sided.c"),
                    "-L", lib, "-lbppp_hip", "-Wl,-rpath," + lib, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "one-sided c client ok" in p.stdout, (p.stdout[-2000:], p.stderr[-2000:])
    assert "row 0: owned, amount 1000000" in p.stdout and "row 1: owned, amount 81985529216486895" in p.stdout
    assert "row 2: foreign" in p.stdout and "row 3: tag only" in p.stdout
