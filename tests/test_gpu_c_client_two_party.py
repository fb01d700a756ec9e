"""examples/c_client/rp_two_party.c: on a seeded 64bit-shaped handle in plain C99 a sender (an input and its change) and a receiver (one output) sign
one transaction together — keys and public nonces exchanged (bppp_rp_excess_keys, bppp_rp_excess_part_nonces), aggregated by the sender
(bppp_rp_excess_part_aggregate), each part signed (bppp_rp_excess_part_sign) and the partials combined (bppp_rp_excess_part_combine).  The 65 bytes
are OK under bppp_rp_excess_verify_keys_each with the aggregated key and under bppp_rp_excess_verify_each against the pool with the fee; with the
receiver's partial altered by one the signature is MISMATCH and bppp_rp_excess_part_verify names the receiver's part alone."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_client_two_party(tmp_path, gpu):
    lib = os.path.join(ROOT, "bulletproofspp_amd", "lib")
    exe = str(tmp_path / "rp_two_party")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_client", "rp_two_party.c"),
                    "-L", lib, "-lbppp_hip", "-Wl,-rpath," + lib, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for line in ("round 1: two keys of 33 bytes, two public nonces of 66 bytes", "aggregate: OK", "round 2: two partials of 32 bytes combined into one signature of 65 bytes",
                 "verify_keys_each: OK under the aggregated key", "verify_each: OK against the pool with the fee",
                 "a partial altered by one: MISMATCH, part_verify names the receiver alone", "two-party c client ok"):
        assert line in p.stdout, (line, p.stdout[-2000:])
