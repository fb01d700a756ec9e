"""The host's share of the many-key scan (csrc/rpscan_keys_plan.hpp: the pass geometry, the merge of hits into the call's (row, key) order with
the cap cut, the recoding of a secret) replayed by a native program (tests/native/scan_keys_check.cpp) built with the address and
undefined-behaviour sanitizers: every (row, key) pair is visited exactly once, no index leaves a carved array, the merged lists equal a sorted
reference for cap below, at and above the hit count, and the recoded halves recompose to the scalar."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_keys_plan_replays(tmp_path):
    exe = str(tmp_path / "scan_keys_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bulletproofspp_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "native", "scan_keys_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("replays ok"), out.stdout + out.stderr
