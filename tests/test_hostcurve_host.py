"""The host window combine on lazy 5 x 52-bit limbs (csrc/hostcurve.hpp; no GPU): field, curve and whole-combine cases against hostmath.hpp's
generic mmul / mpow path, built with g++ and run as a native check (tests/native/hostcurve_check.cpp), plain and under
AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program: the sanitizer runtime is linked in)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "hostcurve_check.cpp")
INC = os.path.join(ROOT, "bulletproofspp_amd", "csrc")
FLAGS = {"plain": ["-O2"],
         "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_hostcurve(tmp_path, build):
    exe = str(tmp_path / ("hostcurve_check_" + build))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", INC] + FLAGS[build] + ["-o", exe, SRC], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
