"""Culprit search cost: bppp_rp_verify_batch_device with proof_status under bisection (the default), the same call with
BPPP_RP_OPT_CULPRITS = 1 (one per-proof pass over a rejected batch), and bppp_rp_verify_each_device alone, on the same device-resident
files, alternated within one process after a warm-up.

  64by64:   4096 proofs, f in {0, 1, 8, 64, 512, 4096} tampered (a changed final-witness scalar) at seeded random positions
  binary:   1024 proofs of the 64 x 64-bit binary shape (norm-linear, conserved), f in {0, 64}
  64bit:    2^14 proofs of the inner-product example, f in {0, 64}

Proofs are made once by the library's prover.  The 64by64 and binary handles prove with comb_budget 0 (no fixed-base comb table: the
per-proof pass takes the registered basis, as on a verify-only node); the 64bit handle builds a small table (comb_bits 12) so that its
2^14 proofs are proved on the device, and its per-proof pass then takes that table.  Bisection with f >= 512 costs seconds per call: those
legs run `--slow-reps` times (default 1) instead of --reps.  Prints one JSON line: per shape and f the wall time of each route (median,
quartiles, min, max, ms) and the statuses' agreement.
   python benchmarks/verify_each_timing.py [--reps N] [--warmup W] [--slow-reps N] [--profile]
--profile: only verify_each at 4096 x 64by64 with f = 64, 20 calls (for one `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse, ctypes as C, json, os, random, statistics, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import bulletproofspp_amd as b
from bulletproofspp_amd import rangeproof as RP, rangeproof_binary as RB

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--slow-reps", type=int, default=1)
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()
EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "examples")
gpu = b.Bppp(0)
backend = RP.GpuBackend(gpu)
points = RP.basis_points(b"test points", 4 + 64 * 64 + 8)


def example(name, comb_bits=0):
    schema = json.load(open(os.path.join(EX, name, "schema.json")))
    wit = json.load(open(os.path.join(EX, name, "witness.json")))
    nat = RP.NativeRangeProofs(gpu, RP.setup_from_schema(backend, schema, points))
    if comb_bits:
        nat.set_option("comb_bits", comb_bits)
    else:
        nat.set_option("comb_budget", 0)
    return nat, lambda j: RP.inputs_from_witness(wit, b"each %d" % j)


def binary64():
    count, amount = 64, 10000
    rds = [RB.make_range_data(0, 2**64, True, False)] * count
    nat = RB.NativeBinaryRangeProofs(gpu, RB.setup(backend, points, True, rds, amount * count, "NL"))
    nat.set_option("comb_budget", 0)
    rng = np.random.default_rng(0xB164)

    def make(j):
        d = [int(x) for x in rng.integers(-5000, 5000, size=count // 2)]
        vals = [amount + x for x in d] + [amount - x for x in d]
        return [(v, int(bl)) for v, bl in zip(vals, rng.integers(1, 2**63, size=count, dtype=np.uint64))]
    return nat, make


def prove(nat, make, B, tag):
    cf, pf = [], []
    for lo in range(0, B, 512):                     # prove batches below 1024 proofs
        n = min(512, B - lo)
        files = nat.prove_batch([make(lo + j) for j in range(n)], [b"%s %06d" % (tag, lo + j) for j in range(n)])
        cf += [c for c, _ in files]; pf += [p for _, p in files]
    return cf, pf


def tamper(nat, pf, f, seed):
    """f proofs with a changed final-witness scalar at seeded random positions"""
    pf = list(pf)
    bad = sorted(random.Random(seed).sample(range(len(pf)), f))
    for i in bad:
        p = bytearray(pf[i]); p[31] ^= 4; pf[i] = bytes(p)
    return pf, bad


def up(bs):
    raw = b"".join(bs)
    return gpu.to_device(np.frombuffer(raw + b"\0" * (-len(raw) % 8), dtype=np.uint8).view(np.uint64))


seed = np.frombuffer(b"\x07" * 32, dtype=np.uint8)
acc = C.c_int(0)


def routes(nat, B, dc, dp):
    st = np.zeros(B, dtype=np.uint32)

    def batch(culprits):
        def run():
            nat.set_option("culprits", culprits)
            rc = gpu.lib.bppp_rp_verify_batch_device(nat.h, B, C.c_void_p(dc), C.c_void_p(dp), C.c_void_p(seed.ctypes.data), C.byref(acc),
                                                     C.c_void_p(st.ctypes.data), None, None)
            gpu._check(rc, "bppp_rp_verify_batch_device")
            return st.copy()
        return run

    def each():
        rc = gpu.lib.bppp_rp_verify_each_device(nat.h, B, C.c_void_p(dc), C.c_void_p(dp), C.c_void_p(st.ctypes.data), None)
        gpu._check(rc, "bppp_rp_verify_each_device")
        return st.copy()
    return {"bisect": batch(0), "pass": batch(1), "each": each}


def stats(ts):
    ts = sorted(t * 1e3 for t in ts)
    q = statistics.quantiles(ts, n=4) if len(ts) >= 2 else [ts[0]] * 3
    return {"median": round(statistics.median(ts), 3), "p25": round(q[0], 3), "p75": round(q[2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3),
            "n": len(ts)}


def measure(nat, cf, pf, fs, tag):
    out = {}
    B = len(pf)
    dc = up(cf)
    for f in fs:
        pft, bad = tamper(nat, pf, f, 1000 + f)
        dp = up(pft)
        rs = routes(nat, B, dc, dp)
        want = np.zeros(B, dtype=np.uint32); want[bad] = 1
        agree = True
        for _ in range(args.warmup):
            for k, fn in rs.items():
                if k == "bisect" and f >= 512:
                    continue
                agree &= bool((fn() == want).all())
        ts = {k: [] for k in rs}
        for r in range(args.reps):
            order = list(rs) if r % 2 == 0 else list(rs)[::-1]         # alternated: drifts hit every route alike
            for k in order:
                if k == "bisect" and f >= 512 and r >= args.slow_reps:
                    continue
                t0 = time.perf_counter(); got = rs[k](); ts[k].append(time.perf_counter() - t0)
                agree &= bool((got == want).all())
        nat.set_option("culprits", 0)
        out["f=%d" % f] = {k: stats(v) for k, v in ts.items()}
        out["f=%d" % f]["statuses_exact"] = agree
        print("[%s] f=%d %s" % (tag, f, {k: out["f=%d" % f][k]["median"] for k in rs}), file=sys.stderr, flush=True)
        gpu.free(dp)
    gpu.free(dc)
    return out


nat64, make64 = example("64by64")
cf64, pf64 = prove(nat64, make64, 4096, b"64by64")
if args.profile:
    pft, _ = tamper(nat64, pf64, 64, 1064)
    dc, dp = up(cf64), up(pft)
    run = routes(nat64, 4096, dc, dp)["each"]
    for _ in range(20):
        run()
    print(json.dumps({"bench": "verify_each_timing", "profile": "20 x verify_each_device, 4096 x 64by64, f = 64"}), flush=True)
    sys.exit(0)
res = {"64by64_4096": measure(nat64, cf64, pf64, [0, 1, 8, 64, 512, 4096], "64by64")}
nat64.close()
natb, makeb = binary64()
cfb, pfb = prove(natb, makeb, 1024, b"bin64")
res["binary64x64_1024"] = measure(natb, cfb, pfb, [0, 64], "binary")
natb.close()
nati, makei = example("64bit", comb_bits=12)
cfi, pfi = prove(nati, makei, 1 << 14, b"64bit")
res["64bit_16384"] = measure(nati, cfi, pfi, [0, 64], "64bit")
nati.close()
print(json.dumps({"bench": "verify_each_timing", "what": "wall ms per call on device-resident files, alternated after warm-up: verify_batch_device with "
                  "proof_status under bisection (bisect) and with culprits = 1 (pass), verify_each_device (each)", "reps": args.reps,
                  "warmup": args.warmup, "slow_reps": args.slow_reps, "results": res}), flush=True)
gpu.close()
