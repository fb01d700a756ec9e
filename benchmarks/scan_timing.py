"""The view-key scan on one 64bit-shaped handle, and its fixed-scalar walk against the quad walk it would otherwise call, in the same run; device
buffers made once outside the timed region, the legs of a step alternated call by call in one process after a warm-up:

  walk16   2^16 points of the seed "scan timing": the lane walk (bppp_test_rp_scan_mul: one lane a point, the scalar a kernel argument, its affine
           launch included) against the quad walk over the same points with the scalar repeated in every row (bppp_test_rp_excess_mul)
  walk20   the same with 2^20 points
  scan16   bppp_rp_scan_device over 2^16 rows of which 16 are sealed to the scanner's key and the rest to another (made by bppp_rp_seal_device
           and bppp_rp_commit_batch_device), all three outputs asked for; next to it the lane walk over the rows' lifted hints, so that
           outside_walk = 1 - walk / scan is the share of a scan spent on the lift, the two hashes, the compaction and the survivors
  scan20   the same with 2^20 rows

Without --step this script is the driver: every step runs as a child process of its own under `timeout` (a step that hangs or faults ends
there and nothing is started after it), and the steps' results are printed as one JSON line.  Wall time of the C call only; median, min
and max over --reps timed calls per leg.  The ship rule of the walk: lane_walk's median below quad_walk's by more than the spread
(max - min) of the two legs, at both sizes.
   python benchmarks/scan_timing.py [--steps walk16,walk20,scan16,scan20] [--reps 10] [--warmup 2] [--step-timeout 600]"""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time

STEPS = {"walk16": 1 << 16, "walk20": 1 << 20, "scan16": 1 << 16, "scan20": 1 << 20}
ap = argparse.ArgumentParser()
ap.add_argument("--steps", default="walk16,walk20,scan16,scan20")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--step-timeout", type=int, default=600)
ap.add_argument("--step", default=None, help="internal: one of " + ", ".join(STEPS))
args = ap.parse_args()

if args.step is None:
    result = {"reps": args.reps, "warmup": args.warmup}
    for step in [s for s in args.steps.split(",") if s]:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode:
            result[step] = {"failed": p.returncode, "stderr": p.stderr[-400:]}
            print(json.dumps(result))
            sys.exit(1)                               # nothing more is started on a GPU after a step that failed
        result[step] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(result))
    sys.exit(0)

sys.path.insert(0, os.getcwd())
import numpy as np
import bulletproofspp_amd as b
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "examples")
gpu = b.Bppp(0)
lib, tl = gpu.lib, capi.load_test_library()
vp = C.c_void_p
nat = RP.NativeRangeProofs(gpu, RP.setup_from_schema(RP.GpuBackend(gpu), json.load(open(os.path.join(EX, "64bit", "schema.json")))))
n = STEPS[args.step]
OWNED = 16
A_SECRET, OTHER_SECRET = 0x0123456789ABCDEF0F1E2D3C4B5A697899AABBCCDDEEFF001122334455667788, 0x201F1E1D1C1B1A191817161514131211100F0E0D0C0B0A090807060504030201
a = capi.int_to_limbs(A_SECRET)


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def run(legs):
    for _ in range(args.warmup):
        for k, fn in legs.items():
            gpu._check(fn(), k)
    ms = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            t = time.perf_counter()
            rc = fn()
            ms[k].append((time.perf_counter() - t) * 1e3)
            gpu._check(rc, k)
    return {k: stats(v) for k, v in ms.items()}


if args.step.startswith("walk"):
    d_pts, _ = gpu.points_from_seed(b"scan timing", n, device=True)
    d_sc = gpu.to_device(np.tile(a, (n, 1)))
    d_lane, d_quad = gpu.alloc(n * 64), gpu.alloc(n * 64)
    out = run({"lane_walk": lambda: tl.bppp_test_rp_scan_mul(nat.h, n, vp(a.ctypes.data), vp(d_pts), vp(d_lane)),
               "quad_walk": lambda: tl.bppp_test_rp_excess_mul(nat.h, n, vp(d_sc), vp(d_pts), vp(d_quad))})
    same = bool(np.array_equal(gpu.download(d_lane, (n, 8)), gpu.download(d_quad, (n, 8))))
    spread = max(out[k]["max"] - out[k]["min"] for k in out)
    print(json.dumps({"points": n, "ms": out, "ratio lane/quad": round(out["lane_walk"]["median"] / out["quad_walk"]["median"], 3), "spread_ms": round(spread, 3),
                      "lane_ships": bool(out["quad_walk"]["median"] - out["lane_walk"]["median"] > spread), "same_points": same}))
    sys.exit(0 if same else 1)

# scan: n rows, OWNED of them sealed to our key at spread-out positions, the rest to another key
nr, sb, cb = 1, RP.SEAL_BYTES(1), nat.shape["coms_bytes"]
keys = nat.excess_keys([A_SECRET, OTHER_SECRET])
own = set(range(n // (2 * OWNED), n, n // OWNED))
vk = np.tile(np.frombuffer(keys[1], dtype=np.uint8), (n, 1))
for r in own:
    vk[r] = np.frombuffer(keys[0], dtype=np.uint8)
rng = np.random.default_rng(0x5CA9)
eph = np.zeros((n, 4), dtype=np.uint64)
eph[:, :3] = rng.integers(1, 2**63, size=(n, 3), dtype=np.uint64)
amt = np.zeros((n, 4), dtype=np.uint64)
amt[:, 0] = rng.integers(0, 2**63, size=n, dtype=np.uint64)
d_vk, d_eph, d_amt, d_typ = gpu.to_device(vk), gpu.to_device(eph), gpu.to_device(amt), gpu.to_device(np.zeros((n, 4), dtype=np.uint64))
d_seals, d_bl, d_coms = gpu.alloc(n * sb), gpu.alloc(n * 32), gpu.alloc(n * cb)
t0 = time.perf_counter()
gpu._check(lib.bppp_rp_seal_device(nat.h, n, vp(d_vk), vp(d_eph), vp(d_amt), vp(d_typ), vp(d_seals), vp(d_bl), None), "seal")
seal_ms = (time.perf_counter() - t0) * 1e3
gpu._check(lib.bppp_rp_commit_batch_device(nat.h, n, vp(d_amt), vp(d_typ), vp(d_bl), None, vp(d_coms)), "commit")
# the hints as affine points, for the walk alone: the first 32 bytes of a seal are put (x); any root serves a timing
seals = gpu.download(d_seals, (n, sb), np.uint8)
xs = np.ascontiguousarray(seals[:, :32].reshape(n, 4, 8)[:, :, ::-1]).view(np.uint64).reshape(n, 4)
d_x, d_R, d_lane = gpu.to_device(xs), gpu.alloc(n * 64), gpu.alloc(n * 64)
gpu.lift_x(d_x, n, d_R)
status, nown = np.zeros(n, dtype=np.uint32), C.c_size_t(0)
d_out = [gpu.alloc(n * 32) for _ in range(3)]
out = run({"scan": lambda: lib.bppp_rp_scan_device(nat.h, vp(a.ctypes.data), n, vp(d_coms), vp(d_seals), vp(status.ctypes.data), vp(d_out[0]), vp(d_out[1]), vp(d_out[2]), C.byref(nown)),
           "lane_walk": lambda: tl.bppp_test_rp_scan_mul(nat.h, n, vp(a.ctypes.data), vp(d_R), vp(d_lane))})
owned_rows = set(int(i) for i in np.nonzero(status == RP.SCAN_OWNED)[0])
got_amt = gpu.download(d_out[0], (n, 4))
ok = owned_rows == own and nown.value == OWNED and all(np.array_equal(got_amt[r], amt[r]) for r in own) and not got_amt[[r for r in range(min(n, 64)) if r not in own]].any()
counts = {name: int((status == code).sum()) for name, code in (("foreign", RP.SCAN_FOREIGN), ("owned", RP.SCAN_OWNED), ("bad_hint", RP.SCAN_BAD_HINT), ("tag_only", RP.SCAN_TAG_ONLY))}
print(json.dumps({"rows": n, "verdicts": counts, "seal_ms_once": round(seal_ms, 3), "ms": out, "rows_per_s": round(n / out["scan"]["median"] * 1e3),
                  "outside_walk": round(1 - out["lane_walk"]["median"] / out["scan"]["median"], 3), "all_true": bool(ok)}))
sys.exit(0 if ok else 1)
