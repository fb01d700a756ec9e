"""examples/c_client/rp_seeded.c: a handle created from the string "test points" (bppp_rp_create_seeded) in plain C99, two proofs proved
and verified, and the first basis point printed — checked here against the inline restatement of getPoints' first point for that seed."""
import hashlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2**256 - 2**32 - 977


def _first_point(seed):
    n = 0
    while True:
        d = hashlib.sha256(seed + str(n).encode()).digest()
        x = sum(int.from_bytes(d[8 * i:8 * i + 8], "big") << (64 * i) for i in range(4)) % P
        rhs = (x * x * x + 7) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs:
            return x, (P - y if y & 1 else y)
        n += 1


def test_c_client_seeded(tmp_path, gpu):
    lib = os.path.join(ROOT, "bulletproofspp_amd", "lib")
    exe = str(tmp_path / "rp_seeded")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_client", "rp_seeded.c"),
                    "-L", lib, "-lbppp_hip", "-Wl,-rpath," + lib, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "seeded c client ok" in p.stdout, (p.stdout[-2000:], p.stderr[-2000:])
    line = [l for l in p.stdout.splitlines() if l.startswith("basis[0] ")]
    assert len(line) == 1
    _, xs, ys = line[0].split()
    assert (int(xs, 16), int(ys, 16)) == _first_point(b"test points")
