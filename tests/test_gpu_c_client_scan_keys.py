"""examples/c_client/rp_scan_keys.c: a seeded handle in plain C99 seals eight outputs — two to each of two accounts, none to a third, four to a
stranger — commits them, and scans them under the three accounts' view secrets in one call (bppp_rp_scan_keys): the hit list is printed in
(row, key) order; then a ninth output is sealed to the third account and found."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_client_scan_keys(tmp_path, gpu):
    lib = os.path.join(ROOT, "bulletproofspp_amd", "lib")
    exe = str(tmp_path / "rp_scan_keys")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_client", "rp_scan_keys.c"),
                    "-L", lib, "-lbppp_hip", "-Wl,-rpath," + lib, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "scan-keys c client ok" in p.stdout, (p.stdout[-2000:], p.stderr[-2000:])
    first, second = p.stdout.split("scan of 9 rows under 3 keys: 5 hits")
    assert "scan of 8 rows under 3 keys: 4 hits" in first
    hits = ["account 0 owns row 1, amount 2000", "account 1 owns row 3, amount 4000", "account 0 owns row 4, amount 5000", "account 1 owns row 6, amount 7000"]
    for part in (first, second):
        assert [part.index(h) for h in hits] == sorted(part.index(h) for h in hits)
    assert "account 2" not in first and "hit 4: account 2 owns row 8, amount 9000" in second
