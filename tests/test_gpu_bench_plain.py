"""bench.py's plain run (`--gpus 1 --steps K --warmup W`): the headline MSM alone, K timed steps, and with --dump-outputs the point
the last step returned — the oracle's Straus sum over the same seeded inputs, regenerated in this process."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_the_last_result(tmp_path, oracle_lib):
    log2n, steps = 12, 3
    out_dir = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--log2n", str(log2n),
           "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["metric"] == "msm_scalar_point_pairs_per_sec" and line["unit"] == "pairs/s" and line["higher_is_better"] is True and line["dtype"]
    assert line["steps"] == steps and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert abs(line["value"] - (1 << log2n) * 1e3 / line["ms_per_step"]) <= 1e-9 * line["value"]
    assert not set(line) & {"cpu_baseline", "valu", "msm_2_16", "msm_fixed_basis", "msm_fixed_basis_batch", "concurrent", "host_buffer_call", "verify", "prove"}
    got = np.load(out_dir / "msm_result.npy")
    assert got.dtype == np.float64 and got.shape == (2, 8)

    import torch
    sys.path.insert(0, ROOT)
    import bench
    import bulletproofspp_amd as b
    from bulletproofspp_amd.capi import array_to_point
    dev = torch.device("cuda", 0)
    gpu = b.Bppp(0)
    try:
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):                      # torch's copies and the library's kernels in one stream, as bench.py runs them
            gpu.set_stream(s.cuda_stream)
            dsc, dpts = bench.make_inputs(gpu, torch, dev, 1 << log2n, seed=0xB9B9)
            sc = np.ascontiguousarray(dsc.cpu().numpy().view(np.uint64))
            pts = np.ascontiguousarray(dpts.cpu().numpy().view(np.uint64))
        torch.cuda.synchronize()
    finally:
        gpu.close()
    u64p = ctypes.POINTER(ctypes.c_uint64)
    want = oracle_lib.inner_product_raw(sc.ctypes.data_as(u64p), pts.ctypes.data_as(u64p), 1 << log2n)
    assert array_to_point(got.astype(np.uint32).reshape(16).view(np.uint64)) == want
