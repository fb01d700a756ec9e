"""examples/c_client/rp_assemble.c: the scenario of rp_cut_through.c with the block's hand-written arrays replaced by ONE bppp_rp_cut_through.  A
seeded 64bit-shaped handle in plain C99 receives two transactions as six rows (A; B, C; B again as tx 2's input; D; E), each balanced against its
own key; the call drops B with its spend, puts the new outputs C and D in front of A and E, re-bases the one sum and adds up fees and offsets;
bppp_rp_excess_sums_each over what it returned is OK, and MISMATCH with a fee off by one."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_client_assemble(tmp_path, gpu):
    lib = os.path.join(ROOT, "bulletproofspp_amd", "lib")
    exe = str(tmp_path / "rp_assemble")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_client", "rp_assemble.c"),
                    "-L", lib, "-lbppp_hip", "-Wl,-rpath," + lib, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for line in ("builders: two transactions", "as received: each transaction balances against its own key", "cut_through: B is gone; 4 rows (2 new outputs in front), 4 entries, 2 cut",
                 "sums_each over the block: OK", "a fee off by one: MISMATCH", "assemble c client ok"):
        assert line in p.stdout, (line, p.stdout[-2000:])
