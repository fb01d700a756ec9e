"""bench.py's command line without a GPU: the --full and --dump-outputs options exist, --steps below 1 is refused before anything
starts, and the file --dump-outputs writes holds the point exactly (32-bit limbs in float64)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_options_and_step_count_check():
    bench = os.path.join(ROOT, "bench.py")
    h = subprocess.run([sys.executable, bench, "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
    p = subprocess.run([sys.executable, bench, "--gpus", "1", "--steps", "0"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr


def test_dump_outputs_holds_the_point_exactly(tmp_path):
    import bench
    from bulletproofspp_amd.capi import array_to_point
    x = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
    y = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
    for pt in ((x, y), None):
        bench.dump_outputs(str(tmp_path / "d"), pt)
        got = np.load(tmp_path / "d" / "msm_result.npy")
        assert got.dtype == np.float64 and got.shape == (2, 8)
        assert array_to_point(got.astype(np.uint32).reshape(16).view(np.uint64)) == pt
