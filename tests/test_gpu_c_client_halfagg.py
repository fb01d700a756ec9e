"""examples/c_client/rp_halfagg.c: the two transactions of rp_cut_through.c in plain C99; their signatures are checked, aggregated to 98 bytes
(bppp_rp_excess_halfagg) and the aggregate is accepted by bppp_rp_excess_halfagg_verify, refused with one message changed (MISMATCH for both keys), and
accepted inside the block after cut-through by bppp_rp_verify_block_agg, which still refuses a fee off by one."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_client_halfagg(tmp_path, gpu):
    lib = os.path.join(ROOT, "bulletproofspp_amd", "lib")
    exe = str(tmp_path / "rp_halfagg")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_client", "rp_halfagg.c"),
                    "-L", lib, "-lbppp_hip", "-Wl,-rpath," + lib, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for line in ("verify_keys_batch: accept", "halfagg: 130 signature bytes became 98", "halfagg_verify: accept", "one message changed: reject, MISMATCH for both keys",
                 "verify_block_agg: accept", "a fee off by one: reject, the sum MISMATCH, the aggregate OK", "halfagg c client ok: two kernels kept as 164 bytes"):
        assert line in p.stdout, (line, p.stdout[-2000:])
