"""witness_status (csrc/rpsetup.hpp) — the host function behind every BPPP_RP_WIT_* verdict of the prover's host-buffer routes and of the
messages of bppp_rp_prove_batch_pub — under AddressSanitizer + UndefinedBehaviorSanitizer (CPU build, tests/native/witness_status_check.cpp):
every reason and the order of precedence on the shapes of examples/rec_test and examples/bin_test."""
import subprocess

from test_host_sanitizers import ASAN, _build


def test_witness_status_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "witness_status_check.cpp", ASAN, "witness_status_check")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok") and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stdout[-3000:] + p.stderr[-3000:]
