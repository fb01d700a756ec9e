"""The host's share of the set commitments (csrc/rpset_plan.hpp: the peak positions, the per-level ranges of new nodes, the passes of an append, the
path layout, the growth of the level arrays) replayed by a native program (tests/native/set_plan_check.cpp) built with the address and
undefined-behaviour sanitizers: an append walked exactly as the kernels index it creates every node of the definition once, from its own children,
and reads nothing that does not exist; the frontier ends as the peaks; paths lie where a plain walk over the peaks puts them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_plan_replays(tmp_path):
    exe = str(tmp_path / "set_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bulletproofspp_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "native", "set_plan_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("replays ok"), out.stdout + out.stderr
