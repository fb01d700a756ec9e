"""The scan under many view secrets against the loop of one-key scans it replaces, on one 64bit-shaped handle; device buffers made once outside the
timed region, the legs of a step alternated call by call in one process after a warm-up.  A step is rows x keys:

  r16k16   2^16 rows, 16 keys       r16k256   2^16 rows, 256 keys       r20k16   2^20 rows, 16 keys       r20k64   2^20 rows, 64 keys

16 rows are sealed to the first key at spread-out positions and the rest to a key that is not in the list (made by bppp_rp_seal_device and
bppp_rp_commit_batch_device); the other keys are seeded and own nothing.  Legs:

  keys        bppp_rp_scan_keys_device, cap = 64, all three outputs asked for
  loop        K sequential bppp_rp_scan_device calls over the same buffers, all three outputs asked for
  walk_keys   the table, the multi-key walk and the batched affine conversion alone over the rows' lifted hints (bppp_test_rp_scan_keys_mul)
  walk_loop   K launches of the one-key walk over the same points (bppp_test_rp_scan_mul)

so that ratio = keys / loop, walk_ratio = walk_keys / walk_loop and outside_walk = 1 - walk_keys / keys (the share of the call spent on the lift,
the hashes, the compaction, the survivors and the host).  The rule for the call: keys' median below loop's by more than the spread (max - min) of
the two legs, at every step.

Without --step this script is the driver: every step runs as a child process of its own under `timeout` (a step that hangs or faults ends
there and nothing is started after it), and the steps' results are printed as one JSON line.  Wall time of the C calls only; median, min and
max over --reps timed calls per leg.
   python benchmarks/scan_keys_timing.py [--steps r16k16,r16k256,r20k16,r20k64] [--reps 10] [--warmup 2] [--step-timeout 900]"""
import argparse, ctypes as C, json, os, random, statistics, subprocess, sys, time

STEPS = {"r16k16": (1 << 16, 16), "r16k256": (1 << 16, 256), "r20k16": (1 << 20, 16), "r20k64": (1 << 20, 64)}
ap = argparse.ArgumentParser()
ap.add_argument("--steps", default="r16k16,r16k256,r20k16,r20k64")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--step-timeout", type=int, default=900)
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
n, K = STEPS[args.step]
OWNED, CAP = 16, 64
A_SECRET, OTHER_SECRET = 0x0123456789ABCDEF0F1E2D3C4B5A697899AABBCCDDEEFF001122334455667788, 0x201F1E1D1C1B1A191817161514131211100F0E0D0C0B0A090807060504030201
rnd = random.Random("scan keys timing")
secrets = [A_SECRET] + [rnd.randrange(1, RP.N) for _ in range(K - 1)]
sec = capi.scalars_to_array(secrets)


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


# n rows, OWNED of them sealed to the first key at spread-out positions, the rest to a key outside the list
nr, sb, cb = 1, RP.SEAL_BYTES(1), nat.shape["coms_bytes"]
keys = nat.excess_keys([A_SECRET, OTHER_SECRET])
own = sorted(range(n // (2 * OWNED), n, n // OWNED))
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
gpu._check(lib.bppp_rp_seal_device(nat.h, n, vp(d_vk), vp(d_eph), vp(d_amt), vp(d_typ), vp(d_seals), vp(d_bl), None), "seal")
gpu._check(lib.bppp_rp_commit_batch_device(nat.h, n, vp(d_amt), vp(d_typ), vp(d_bl), None, vp(d_coms)), "commit")
# the hints as affine points, for the walks alone: the first 32 bytes of a seal are put (x); any root serves a timing
seals = gpu.download(d_seals, (n, sb), np.uint8)
xs = np.ascontiguousarray(seals[:, :32].reshape(n, 4, 8)[:, :, ::-1]).view(np.uint64).reshape(n, 4)
d_x, d_R = gpu.to_device(xs), gpu.alloc(n * 64)
gpu.lift_x(d_x, n, d_R)
d_walk_keys, d_walk_one = gpu.alloc(K * n * 64), gpu.alloc(n * 64)
row_status, one_status = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
hk, hr = np.zeros(CAP, dtype=np.uint32), np.zeros(CAP, dtype=np.uint32)
nhits, ntag, nown = C.c_size_t(0), C.c_uint64(0), C.c_size_t(0)
d_hit = [gpu.alloc(CAP * 32) for _ in range(3)]
d_out = [gpu.alloc(n * 32) for _ in range(3)]
loop_owned = [0] * K


def loop():
    for k in range(K):
        rc = lib.bppp_rp_scan_device(nat.h, vp(sec[k].ctypes.data), n, vp(d_coms), vp(d_seals), vp(one_status.ctypes.data), vp(d_out[0]), vp(d_out[1]), vp(d_out[2]), C.byref(nown))
        if rc:
            return rc
        loop_owned[k] = nown.value
    return 0


def walk_loop():
    for k in range(K):
        rc = tl.bppp_test_rp_scan_mul(nat.h, n, vp(sec[k].ctypes.data), vp(d_R), vp(d_walk_one))
        if rc:
            return rc
    return 0


out = run({"keys": lambda: lib.bppp_rp_scan_keys_device(nat.h, K, vp(sec.ctypes.data), n, vp(d_coms), vp(d_seals), vp(row_status.ctypes.data), CAP, vp(hk.ctypes.data), vp(hr.ctypes.data),
                                                        vp(d_hit[0]), vp(d_hit[1]), vp(d_hit[2]), C.byref(nhits), C.byref(ntag)),
           "loop": loop,
           "walk_keys": lambda: tl.bppp_test_rp_scan_keys_mul(nat.h, K, vp(sec.ctypes.data), n, vp(d_R), vp(d_walk_keys)),
           "walk_loop": walk_loop})
# the last key's walk of the loop is still in its buffer: the multi-key walk's last row block must equal it
same = bool(np.array_equal(gpu.download(d_walk_one, (n, 8)), gpu.download(d_walk_keys + (K - 1) * n * 64, (n, 8))))
got_amt = gpu.download(d_hit[0], (CAP, 4))
ok = (nhits.value == OWNED and [int(r) for r in hr[:OWNED]] == own and not hk[:OWNED].any() and all(np.array_equal(got_amt[h], amt[r]) for h, r in enumerate(own))
      and not got_amt[OWNED:].any() and int((row_status == RP.SCAN_OWNED).sum()) == OWNED and loop_owned == [OWNED] + [0] * (K - 1) and same)
spread = max(out[k]["max"] - out[k]["min"] for k in ("keys", "loop"))
print(json.dumps({"rows": n, "keys": K, "hits": int(nhits.value), "tag_only_pairs": int(ntag.value), "ms": out, "ratio keys/loop": round(out["keys"]["median"] / out["loop"]["median"], 3),
                  "walk_ratio": round(out["walk_keys"]["median"] / out["walk_loop"]["median"], 3), "spread_ms": round(spread, 3),
                  "keys_wins": bool(out["loop"]["median"] - out["keys"]["median"] > spread), "outside_walk": round(1 - out["walk_keys"]["median"] / out["keys"]["median"], 3),
                  "pairs_per_s": round(n * K / out["keys"]["median"] * 1e3), "all_true": bool(ok)}))
sys.exit(0 if ok else 1)
