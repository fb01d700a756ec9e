"""examples/c_client/rp_set.c: a seeded 64bit-shaped handle in plain C99 commits six outputs and appends their commitments files to a set in two calls;
a full store, a frontier-only set and one restored from the peaks in between print one root; the path of output 2 is accepted under it and refused
under the root before the second append and with a row byte changed.  The example checks every verdict itself; here its lines are read: two
different roots of 32 bytes, then the acceptance and the two refusals in order."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_client_set(tmp_path, gpu):
    lib = os.path.join(ROOT, "bulletproofspp_amd", "lib")
    exe = str(tmp_path / "rp_set")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_client", "rp_set.c"),
                    "-L", lib, "-lbppp_hip", "-Wl,-rpath," + lib, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "set c client ok" in p.stdout, (p.stdout[-2000:], p.stderr[-2000:])
    roots = re.findall(r"root after (\d) rows: ([0-9a-f]{64})\n", p.stdout)
    assert [r[0] for r in roots] == ["4", "6"] and roots[0][1] != roots[1][1]
    order = ["path of row 2 among 6: 96 bytes, accepted", "the same path under the root of 4 rows: refused", "a row with one byte changed: refused"]
    assert [p.stdout.index(s) for s in order] == sorted(p.stdout.index(s) for s in order)
