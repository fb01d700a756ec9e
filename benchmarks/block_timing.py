"""bppp_rp_verify_block_device against the three calls it folds into one MSM, over the same device buffers, in the same run.

One 64bit-shaped handle; a block after cut-through as ONE sum: P proven outputs (proofs from the native prover, bound to 32-byte transaction
messages), P inputs, P / 2 keys with signatures, one summed fee and one summed offset.

  block  bppp_rp_verify_block_device: one MSM
  three  bppp_rp_verify_bound_device, bppp_rp_excess_verify_keys_batch_device and bppp_rp_excess_sums_batch_device in sequence: three MSMs.
         These calls are code the block call did not change, so this column stands for the library without it.

Without --step this script is the driver: every size runs as a child process of its own under `timeout` (a step that hangs or faults ends there
and nothing is started after it), and the steps' results are printed as one JSON line.  Device buffers are uploaded once outside the timed region,
the legs alternated call by call in one process after a warm-up; wall time of the C calls only; median, min and max over --reps timed calls per
leg.  No pass mark.  Every step ends with one block call under the handle's TIMING option, whose stage times (stderr) are reported as "stages".
   python benchmarks/block_timing.py [--sizes 256,4096] [--reps 10] [--warmup 2] [--step-timeout 600]"""
import argparse, ctypes as C, hashlib, json, os, random, statistics, subprocess, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="256,4096")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--step-timeout", type=int, default=600)
ap.add_argument("--step", type=int, default=None, help="internal: P of one step")
args = ap.parse_args()

if args.step is None:
    result = {"reps": args.reps, "warmup": args.warmup}
    for P in [int(s) for s in args.sizes.split(",") if s]:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", str(P), "--reps", str(args.reps), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode:
            result["P=%d" % P] = {"failed": p.returncode, "stderr": p.stderr[-400:]}
            print(json.dumps(result))
            sys.exit(1)                               # nothing more is started on a GPU after a step that failed
        result["P=%d" % P] = json.loads(p.stdout.strip().splitlines()[-1])
        result["P=%d" % P]["stages"] = [" ".join(l.split()[1:]) for l in p.stderr.splitlines() if l.startswith("[rp_verify_block]")]
    print(json.dumps(result))
    sys.exit(0)

sys.path.insert(0, os.getcwd())
import numpy as np
import bulletproofspp_amd as b
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "examples")
gpu = b.Bppp(0)
lib = gpu.lib
vp = C.c_void_p
nat = RP.NativeRangeProofs(gpu, RP.setup_from_schema(RP.GpuBackend(gpu), json.load(open(os.path.join(EX, "64bit", "schema.json")))))
P = args.step
NK = P // 2
rnd = random.Random(0xB10C + P)
bl = lambda: rnd.randrange(1, 2**250)
outs = [[(rnd.randrange(2**40), 0, bl())] for _ in range(P)]
ins = [[(rnd.randrange(2**41), 0, bl())] for _ in range(P)]
ks = [bl() for _ in range(NK)]
bindings = [hashlib.sha256(b"block timing tx %d" % (j // 2)).digest() for j in range(P)]
files = nat.prove_batch(outs, [b"block timing rnd %06d" % j for j in range(P)], bindings=bindings)
coms = [c for c, _ in files] + nat.commit_batch(ins)
SUB = RP.TALLY_SUBTRACT
entries = list(range(P)) + [j | SUB for j in range(P, 2 * P)]
# the claim of the one sum: outputs - inputs less the keys' scalars (witness rows of amount zero), so the blinding claim is the revealed offset
claim = nat.tally_claims(outs + ins + [[(0, 0, k)] for k in ks], [0, 2 * P + NK], entries + [j | SUB for j in range(2 * P, 2 * P + NK)])
msgs = [hashlib.sha256(b"block timing msg %d" % k).digest() for k in range(NK)]
keys, sigs = nat.excess_keys(ks), nat.excess_sign(ks, msgs, hashlib.sha256(b"block timing aux").digest())
arrs, n = nat.block_arrays(coms, [p for _, p in files], [0, 2 * P], entries, claim, [0, NK], keys, msgs, sigs, bindings)
blk = capi.RpBlock(**n)
d = {}
for name, a in arrs:
    d[name] = gpu.to_device(a)
    setattr(blk, name, d[name])
seed = np.frombuffer(os.urandom(32), dtype=np.uint8)
s0, s1, s2 = (np.frombuffer(s, dtype=np.uint8) for s in RP.block_seeds(seed.tobytes()))
acc = [C.c_int(0) for _ in range(4)]


def three():
    rc = lib.bppp_rp_verify_bound_device(nat.h, P, 0, vp(d["coms_files"]), vp(d["proof_files"]), None, vp(d["bindings"]), vp(s0.ctypes.data), C.byref(acc[1]), None, None, None)
    rc = rc or lib.bppp_rp_excess_verify_keys_batch_device(nat.h, NK, vp(d["keys"]), vp(d["msgs"]), vp(d["sigs"]), 0, vp(s1.ctypes.data), C.byref(acc[2]), None, None)
    return rc or lib.bppp_rp_excess_sums_batch_device(nat.h, 2 * P, vp(d["coms_files"]), 1, vp(d["sum_start"]), vp(d["entries"]), 2 * P, vp(d["claim_amounts"]),
                                                      vp(d["claim_types"]), vp(d["claim_offsets"]), NK, vp(d["key_start"]), vp(d["keys"]), 0, vp(s2.ctypes.data), C.byref(acc[3]),
                                                      None, None)


legs = {"block": lambda: lib.bppp_rp_verify_block_device(nat.h, C.byref(blk), vp(seed.ctypes.data), C.byref(acc[0]), None, None), "three": three}


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


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
out = {k: stats(v) for k, v in ms.items()}
ok = all(a.value == 1 for a in acc)
cnt = [C.c_uint64(0) for _ in range(4)]
gpu._check(legs["block"](), "block")
capi.load_test_library().bppp_test_rp_last_block_counts(nat.h, *[C.byref(x) for x in cnt])
sh = nat.shape
basis, per = 1 + sh["lin_len"] + sh["norm_len"], 4 + 1 + 2 * sh["rounds"]
proof_points = P * (4 + 2 * sh["rounds"])                     # the points of the proof files: lifted once on either side
terms = {"block": int(cnt[1].value), "three": [basis + P * per, 2 * NK + 1, 2 * P + NK + 3]}
# square roots: commitments, keys and the signatures' R, next to the proof files' own points
roots = {"block": int(cnt[3].value) + int(cnt[2].value) + NK + proof_points, "three": (P + 2 * P) + 2 * NK + NK + proof_points}
nat.set_option("timing", 1)
gpu._check(legs["block"](), "block")
nat.set_option("timing", 0)
print(json.dumps({"P": P, "inputs": P, "keys": NK, "ms": out, "ratio block/three": round(out["block"]["median"] / out["three"]["median"], 3), "msms": {"block": int(cnt[0].value), "three": 3},
                  "terms": terms, "square_roots": roots, "all_accept": bool(ok)}))
sys.exit(0 if ok else 1)
