"""The half-aggregate calls on one 64bit-shaped handle against the seeded calls they stand next to, in the same run; device buffers uploaded once
outside the timed region, the legs of a step alternated call by call in one process after a warm-up:

  keys12     2^12 kernels: bppp_rp_excess_halfagg_device (the aggregator) and bppp_rp_excess_halfagg_verify_device over (key, message, aggregate),
             against bppp_rp_excess_verify_keys_batch_device over (key, message, signature)
  keys16     the same with 2^16 kernels
  block256   bppp_rp_verify_block_agg_device against bppp_rp_verify_block_device over benchmarks/block_timing.py's block of P = 256 proven outputs,
             P inputs and P / 2 kernels: the same buffers, the aggregate in place of the signatures
  block4096  the same with P = 4096

Without --step this script is the driver: every step runs as a child process of its own under `timeout` (a step that hangs or faults ends
there and nothing is started after it), and the steps' results are printed as one JSON line.  Wall time of the C call only; median, min
and max over --reps timed calls per leg, and the ratios of the medians.  No pass mark: the aggregate is a capability, and the comparison says
what it costs next to the seeded batch.
   python benchmarks/halfagg_timing.py [--steps keys12,keys16,block256,block4096] [--reps 10] [--warmup 2] [--step-timeout 600]"""
import argparse, ctypes as C, hashlib, json, os, random, statistics, subprocess, sys, time

STEPS = {"keys12": 1 << 12, "keys16": 1 << 16, "block256": 256, "block4096": 4096}
ap = argparse.ArgumentParser()
ap.add_argument("--steps", default="keys12,keys16,block256,block4096")
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
lib = gpu.lib
vp = C.c_void_p
nat = RP.NativeRangeProofs(gpu, RP.setup_from_schema(RP.GpuBackend(gpu), json.load(open(os.path.join(EX, "64bit", "schema.json")))))
SIG, KEY, AGG = RP.EXCESS_SIG_BYTES, RP.EXCESS_KEY_BYTES, RP.EXCESS_AGG_BYTES
seed = np.frombuffer(os.urandom(32), dtype=np.uint8)


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


if args.step.startswith("keys"):
    nkeys = STEPS[args.step]
    rng = np.random.default_rng(0xA66)
    bld = np.zeros((nkeys, 4), dtype=np.uint64)
    bld[:, 0] = rng.integers(1, 2**63, size=nkeys, dtype=np.uint64)
    bld[:, 1] = rng.integers(1, 2**63, size=nkeys, dtype=np.uint64)
    aux = np.frombuffer(os.urandom(32), dtype=np.uint8)
    d_bld, d_msg = gpu.to_device(bld), gpu.to_device(rng.integers(0, 256, size=nkeys * 32, dtype=np.uint8))
    d_sig, d_keys, d_agg = gpu.alloc(nkeys * SIG + 16), gpu.alloc(nkeys * KEY + 16), gpu.alloc(AGG(nkeys) + 16)
    sstat, kstat, astat = (np.ones(nkeys, dtype=np.uint32) for _ in range(3))
    gpu._check(lib.bppp_rp_excess_sign_device(nat.h, nkeys, vp(d_bld), vp(d_msg), vp(aux.ctypes.data), vp(d_sig), None, vp(sstat.ctypes.data)), "excess_sign")
    gpu._check(lib.bppp_rp_excess_keys_device(nat.h, nkeys, vp(d_bld), vp(d_keys), vp(kstat.ctypes.data)), "excess_keys")
    gpu._check(lib.bppp_rp_excess_halfagg_device(nat.h, nkeys, vp(d_keys), vp(d_msg), vp(d_sig), vp(d_agg), vp(astat.ctypes.data)), "excess_halfagg")
    acc = [C.c_int(0) for _ in range(2)]
    out = run({"halfagg": lambda: lib.bppp_rp_excess_halfagg_device(nat.h, nkeys, vp(d_keys), vp(d_msg), vp(d_sig), vp(d_agg), None),
               "halfagg_verify": lambda: lib.bppp_rp_excess_halfagg_verify_device(nat.h, nkeys, vp(d_keys), vp(d_msg), vp(d_agg), C.byref(acc[0]), None, None),
               "verify_keys_batch": lambda: lib.bppp_rp_excess_verify_keys_batch_device(nat.h, nkeys, vp(d_keys), vp(d_msg), vp(d_sig), 0, vp(seed.ctypes.data), C.byref(acc[1]), None,
                                                                                        None)})
    ok = acc[0].value == 1 and acc[1].value == 1 and not (sstat.any() or kstat.any() or astat.any())
    ratios = {"halfagg/verify_keys_batch": round(out["halfagg"]["median"] / out["verify_keys_batch"]["median"], 3),
              "halfagg_verify/verify_keys_batch": round(out["halfagg_verify"]["median"] / out["verify_keys_batch"]["median"], 3)}
    print(json.dumps({"keys": nkeys, "bytes": {"signatures": nkeys * SIG, "aggregate": AGG(nkeys)}, "ms": out, "ratios": ratios, "all_true": bool(ok)}))
    sys.exit(0 if ok else 1)

# benchmarks/block_timing.py's block: P proven outputs bound to transaction messages, P inputs, P / 2 kernels, one summed fee and one summed offset
P = STEPS[args.step]
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
claim = nat.tally_claims(outs + ins + [[(0, 0, k)] for k in ks], [0, 2 * P + NK], entries + [j | SUB for j in range(2 * P, 2 * P + NK)])
msgs = [hashlib.sha256(b"block timing msg %d" % k).digest() for k in range(NK)]
keys, sigs = nat.excess_keys(ks), nat.excess_sign(ks, msgs, hashlib.sha256(b"block timing aux").digest())
agg = nat.excess_halfagg(keys, msgs, sigs)
arrs, n = nat.block_arrays(coms, [p for _, p in files], [0, 2 * P], entries, claim, [0, NK], keys, msgs, sigs, bindings)
blk, blk_agg = capi.RpBlock(**n), capi.RpBlock(**n)
for name, a in arrs:
    ptr = gpu.to_device(a)
    setattr(blk, name, ptr)
    if name != "sigs":
        setattr(blk_agg, name, ptr)
d_agg = gpu.to_device(np.frombuffer(agg, dtype=np.uint8))
acc = [C.c_int(0) for _ in range(2)]
out = run({"block_agg": lambda: lib.bppp_rp_verify_block_agg_device(nat.h, C.byref(blk_agg), vp(d_agg), vp(seed.ctypes.data), C.byref(acc[0]), None, None),
           "block": lambda: lib.bppp_rp_verify_block_device(nat.h, C.byref(blk), vp(seed.ctypes.data), C.byref(acc[1]), None, None)})
ok = all(a.value == 1 for a in acc)
print(json.dumps({"P": P, "inputs": P, "keys": NK, "bytes": {"signatures": NK * SIG, "aggregate": AGG(NK)}, "ms": out,
                  "ratio block_agg/block": round(out["block_agg"]["median"] / out["block"]["median"], 3), "all_accept": bool(ok)}))
sys.exit(0 if ok else 1)
