"""The stated-key calls on one 64by64 handle against the calls they stand next to, in the same run; device buffers uploaded once outside the
timed region, the legs of a step alternated call by call in one process after a warm-up:

  keys12  2^12 signatures: bppp_rp_excess_verify_keys_each_device / _batch_device over (key, message, signature) alone, against
          bppp_rp_excess_verify_each_device / _batch_device over the same signatures as one-entry sums of a pool of as many commitments
  keys16  the same with 2^16 signatures
  block   bppp_rp_excess_sums_batch_device of one sum with 2^20 entries and 2^16 stated keys, against bppp_rp_tally_batch_device over the
          entries alone (the blinding sum revealed); the offset is the blinding sum less the keys' scalars, so both sums are true

Without --step this script is the driver: every step runs as a child process of its own under `timeout` (a step that hangs or faults ends
there and nothing is started after it), and the steps' results are printed as one JSON line.  Wall time of the C call only; median, min
and max over --reps timed calls per leg, and the ratios of the medians.  No pass mark.
   python benchmarks/excess_keys_timing.py [--steps keys12,keys16,block] [--reps 10] [--warmup 2] [--step-timeout 600]"""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time

STEPS = {"keys12": 1 << 12, "keys16": 1 << 16, "block": 1 << 16}
ap = argparse.ArgumentParser()
ap.add_argument("--steps", default="keys12,keys16,block")
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
from bulletproofspp_amd import rangeproof as RP

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "examples")
gpu = b.Bppp(0)
lib = gpu.lib
vp = C.c_void_p
nat = RP.NativeRangeProofs(gpu, RP.setup_from_schema(RP.GpuBackend(gpu), json.load(open(os.path.join(EX, "64by64", "schema.json")))))
NR, CB, SIG, KEY = 64, nat.shape["coms_bytes"], RP.EXCESS_SIG_BYTES, RP.EXCESS_KEY_BYTES


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


nkeys = STEPS[args.step]
nnz = (1 << 20) if args.step == "block" else nkeys          # commitments of the pool, every one an entry
W = nnz + (nkeys if args.step == "block" else 0)             # witness rows: the pool's, then (block) one of amount zero per key, its blinding the key's scalar
B, BW = nnz // NR, W // NR
rng = np.random.default_rng(0x7B)
amt, typ, bld = (np.zeros((W, 4), dtype=np.uint64) for _ in range(3))
amt[:nnz, 0] = rng.integers(0, 2**40, size=nnz, dtype=np.uint64)
bld[:, 0] = rng.integers(1, 2**63, size=W, dtype=np.uint64)
bld[:, 1] = rng.integers(1, 2**63, size=W, dtype=np.uint64)
d_amt, d_typ, d_bld = (gpu.to_device(a) for a in (amt, typ, bld))
d_cf = gpu.alloc(B * CB + 16)
gpu._check(lib.bppp_rp_commit_batch_device(nat.h, B, vp(d_amt), vp(d_typ), vp(d_bld), None, vp(d_cf)), "commit")
seed = np.frombuffer(os.urandom(32), dtype=np.uint8)
aux = np.frombuffer(os.urandom(32), dtype=np.uint8)
acc = [C.c_int(0) for _ in range(2)]

if args.step == "block":
    # the tally's job: one sum of every commitment; the keys' job: the same sum with the keys' rows subtracted, whose blinding claim is the offset
    d_ss, d_en = gpu.to_device(np.array([0, nnz], dtype=np.uint32)), gpu.to_device(np.arange(nnz, dtype=np.uint32))
    full = np.arange(W, dtype=np.uint32)
    full[nnz:] |= np.uint32(1 << 31)
    d_ssw, d_enw = gpu.to_device(np.array([0, W], dtype=np.uint32)), gpu.to_device(full)
    claim = [gpu.alloc(32 + 16) for _ in range(6)]
    gpu._check(lib.bppp_rp_tally_claims_device(nat.h, B, vp(d_amt), vp(d_typ), vp(d_bld), 1, vp(d_ss), vp(d_en), nnz, *(vp(c) for c in claim[:3])), "tally_claims")
    gpu._check(lib.bppp_rp_tally_claims_device(nat.h, BW, vp(d_amt), vp(d_typ), vp(d_bld), 1, vp(d_ssw), vp(d_enw), W, *(vp(c) for c in claim[3:])), "tally_claims (offset)")
    d_keys, kstat = gpu.alloc(nkeys * KEY + 16), np.ones(nkeys, dtype=np.uint32)
    gpu._check(lib.bppp_rp_excess_keys_device(nat.h, nkeys, vp(d_bld + nnz * 32), vp(d_keys), vp(kstat.ctypes.data)), "excess_keys")
    d_ks = gpu.to_device(np.array([0, nkeys], dtype=np.uint32))
    out = run({"sums_batch": lambda: lib.bppp_rp_excess_sums_batch_device(nat.h, B, vp(d_cf), 1, vp(d_ss), vp(d_en), nnz, vp(claim[3]), vp(claim[4]), vp(claim[5]), nkeys, vp(d_ks),
                                                                          vp(d_keys), 0, vp(seed.ctypes.data), C.byref(acc[0]), None, None),
               "tally_batch": lambda: lib.bppp_rp_tally_batch_device(nat.h, B, vp(d_cf), 1, vp(d_ss), vp(d_en), nnz, vp(claim[0]), vp(claim[1]), vp(claim[2]), 0,
                                                                     vp(seed.ctypes.data), C.byref(acc[1]), None, None)})
    ok = acc[0].value == 1 and acc[1].value == 1 and not kstat.any()
    ratios = {"sums_batch/tally_batch": round(out["sums_batch"]["median"] / out["tally_batch"]["median"], 3)}
    print(json.dumps({"entries": nnz, "keys": nkeys, "ms": out, "ratios": ratios, "all_true": bool(ok)}))
    sys.exit(0 if ok else 1)

# one-entry sums: sum t is commitment t, its claim the commitment's own amount and type, its blinding the signing key
d_ss, d_en = gpu.to_device(np.arange(nkeys + 1, dtype=np.uint32)), gpu.to_device(np.arange(nkeys, dtype=np.uint32))
d_ca, d_ct, d_cb = (gpu.alloc(nkeys * 32 + 16) for _ in range(3))
gpu._check(lib.bppp_rp_tally_claims_device(nat.h, B, vp(d_amt), vp(d_typ), vp(d_bld), nkeys, vp(d_ss), vp(d_en), nnz, vp(d_ca), vp(d_ct), vp(d_cb)), "tally_claims")
d_msg, d_sig, d_keys = gpu.to_device(rng.integers(0, 256, size=nkeys * 32, dtype=np.uint8)), gpu.alloc(nkeys * SIG + 16), gpu.alloc(nkeys * KEY + 16)
sstat, kstat, estat, pstat = (np.ones(nkeys, dtype=np.uint32) for _ in range(4))
gpu._check(lib.bppp_rp_excess_sign_device(nat.h, nkeys, vp(d_cb), vp(d_msg), vp(aux.ctypes.data), vp(d_sig), None, vp(sstat.ctypes.data)), "excess_sign")
gpu._check(lib.bppp_rp_excess_keys_device(nat.h, nkeys, vp(d_cb), vp(d_keys), vp(kstat.ctypes.data)), "excess_keys")
out = run({"verify_keys_each": lambda: lib.bppp_rp_excess_verify_keys_each_device(nat.h, nkeys, vp(d_keys), vp(d_msg), vp(d_sig), vp(estat.ctypes.data)),
           "verify_keys_batch": lambda: lib.bppp_rp_excess_verify_keys_batch_device(nat.h, nkeys, vp(d_keys), vp(d_msg), vp(d_sig), 0, vp(seed.ctypes.data), C.byref(acc[0]), None, None),
           "verify_each": lambda: lib.bppp_rp_excess_verify_each_device(nat.h, B, vp(d_cf), nkeys, vp(d_ss), vp(d_en), nnz, vp(d_ca), vp(d_ct), vp(d_msg), vp(d_sig),
                                                                        vp(pstat.ctypes.data), None),
           "verify_batch": lambda: lib.bppp_rp_excess_verify_batch_device(nat.h, B, vp(d_cf), nkeys, vp(d_ss), vp(d_en), nnz, vp(d_ca), vp(d_ct), vp(d_msg), vp(d_sig), 0,
                                                                          vp(seed.ctypes.data), C.byref(acc[1]), None, None)})
ok = acc[0].value == 1 and acc[1].value == 1 and not (sstat.any() or kstat.any() or estat.any() or pstat.any())
ratios = {"verify_keys_each/verify_each": round(out["verify_keys_each"]["median"] / out["verify_each"]["median"], 3),
          "verify_keys_batch/verify_batch": round(out["verify_keys_batch"]["median"] / out["verify_batch"]["median"], 3)}
print(json.dumps({"keys": nkeys, "pool_commitments": nnz, "ms": out, "ratios": ratios, "all_true": bool(ok)}))
sys.exit(0 if ok else 1)
