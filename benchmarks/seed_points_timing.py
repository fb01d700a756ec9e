"""bppp_points_from_seed_device: a setup's basis from its seed (getPoints, app/Main.hs:68-72) into HBM, at the sizes a caller meets —
774 points (the 64by64 example's 2 + linLen + nrmLen is of that order), 4099 (64 binary outputs of 64 bits), 2^16 and 2^20 (a Pedersen
basis) — from the seed of every reference example, "test points".  Wall time of the C call (it ends in a stream synchronise: the pass
record is read back), output buffer allocated once outside the timed region, the sizes alternated call by call after a warm-up; median,
min and max over --reps calls per size.  Against rangeproof.basis_points (Python, one host core, one modular exponentiation per candidate)
at 4099 points, timed --cpu-reps times in the same run; the two results are compared point by point.  Prints one JSON line.
   python benchmarks/seed_points_timing.py [--reps 20] [--warmup 3] [--cpu-reps 3] [--sizes 774,4099,65536,1048576]"""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import bulletproofspp_amd as b
from bulletproofspp_amd import capi, rangeproof as RP

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--cpu-reps", type=int, default=3)
ap.add_argument("--cpu-points", type=int, default=4099)
ap.add_argument("--sizes", default="774,4099,65536,1048576")
args = ap.parse_args()
SEED = b"test points"
sizes = [int(s) for s in args.sizes.split(",")]
gpu = b.Bppp(0)
lib = gpu.lib
d_out = gpu.alloc(max(sizes) * 64)
nxt = {n: C.c_uint64(0) for n in sizes}


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def call(n):
    return lib.bppp_points_from_seed_device(gpu.h, SEED, len(SEED), 0, n, C.c_void_p(d_out), C.byref(nxt[n]))


for _ in range(args.warmup):
    for n in sizes:
        gpu._check(call(n), "warm-up %d" % n)
ms = {n: [] for n in sizes}
for _ in range(args.reps):
    for n in sizes:
        t = time.perf_counter()
        rc = call(n)
        ms[n].append((time.perf_counter() - t) * 1e3)
        gpu._check(rc, "points_from_seed_device %d" % n)
result = {"seed": SEED.decode(), "reps": args.reps, "warmup": args.warmup,
          "gpu_ms": {str(n): dict(stats(ms[n]), candidates=int(nxt[n].value)) for n in sizes}}

if args.cpu_reps:
    n = args.cpu_points
    cpu = []
    for _ in range(args.cpu_reps):
        t = time.perf_counter()
        want = RP.basis_points(SEED, n)
        cpu.append((time.perf_counter() - t) * 1e3)
    got, _ = gpu.points_from_seed(SEED, n)
    assert [capi.array_to_point(r) for r in got] == want, "device stream differs from rangeproof.basis_points"
    result["cpu_basis_points_ms"] = {str(n): stats(cpu)}
    if n in ms:
        result["speedup_at_%d" % n] = round(statistics.median(cpu) / statistics.median(ms[n]), 1)
gpu.free(d_out)
gpu.close()
print(json.dumps(result))
