"""examples/c_client/rp_block.c: rp_cut_through.c's block — two transactions, B created and spent inside it — validated by ONE bppp_rp_verify_block:
the range proofs of C and D bound to their transactions, the two kernel signatures against their stated keys and the balance after cut-through, in one
MSM.  The block is accepted; a fee off by one, a proof under the other transaction's binding and a signature under the other key are each rejected,
and the right one of the three status arrays names the culprit."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_client_block(tmp_path, gpu):
    lib = os.path.join(ROOT, "bulletproofspp_amd", "lib")
    exe = str(tmp_path / "rp_block")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_client", "rp_block.c"),
                    "-L", lib, "-lbppp_hip", "-Wl,-rpath," + lib, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for line in ("builders: two bound proofs, two keys, two signatures, one summed offset", "verify_block: accept", "a fee off by one: reject, sum_status MISMATCH",
                 "a proof under the other binding: reject, proof_status INVALID", "a signature under the other key: reject, key_status MISMATCH", "block c client ok"):
        assert line in p.stdout, (line, p.stdout[-2000:])
