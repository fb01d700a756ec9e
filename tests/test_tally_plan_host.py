"""The host's plan of a tally (csrc/rptally_plan.hpp: the passes over the workspace and the workgroup items of the long sums, level by
level) replayed on integers by a native program (tests/native/tally_plan_check.cpp) built with the address and undefined-behaviour
sanitizers: every sum's slot is written exactly once with the signed sum of its entries, and no index leaves a planned buffer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tally_plan_replays(tmp_path):
    exe = str(tmp_path / "tally_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bulletproofspp_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "native", "tally_plan_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("replays ok"), out.stdout + out.stderr
