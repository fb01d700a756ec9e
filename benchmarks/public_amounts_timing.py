"""Per-proof public amounts (bppp_rp_*_pub) against the fixed-amount calls and against today's workaround, on device-resident files,
repetitions alternated within one process after a warm-up, medians reported.

  leg 1  verify: bppp_rp_verify_batch_pub_device over B proofs with B distinct public amounts (the amounts in HBM) against
         bppp_rp_verify_batch_device over B proofs of one fixed amount, for two typed conserved shapes:
           2x2by64   2 inputs + 2 outputs of 64 bits, a public fee (output)
           128by64   BASELINE config 4: 128 x 64-bit outputs, typed, a public input
  leg 2  the workaround: bppp_rp_verify_mixed_device over one handle per distinct amount (16 and 64 amounts, B / k proofs each; the
         handles' creation timed on its own), on the same proofs as leg 1's _pub call
  leg 3  prove: bppp_rp_prove_batch_pub (B distinct amounts) against bppp_rp_prove_batch (one amount), 2x2by64

Prints one JSON line (ms: median, min, max per route).
   python benchmarks/public_amounts_timing.py [--batch 4096] [--reps 9] [--warmup 2] [--prove-reps 3] [--skip-128]"""
import argparse, json, os, statistics, sys, time, zlib
sys.path.insert(0, os.getcwd())
import numpy as np
import bulletproofspp_amd as b
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd.capi import scalars_to_array

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--prove-reps", type=int, default=3)
ap.add_argument("--skip-128", action="store_true")
args = ap.parse_args()
B = args.batch
EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "examples")
gpu = b.Bppp(0)
backend = RP.GpuBackend(gpu)
SEED = b"\x5a" * 32


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def timed(fn):
    t = time.perf_counter(); r = fn(); return (time.perf_counter() - t) * 1e3, r


def alternate(routes, reps, warmup):
    """routes: {name: fn}; every rep runs each route once, in turn"""
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    out = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            ms, r = timed(fn)
            assert r, k
            out[k].append(ms)
    return {k: stats(v) for k, v in out.items()}


def up(bs):
    raw = b"".join(bs)
    return gpu.to_device(np.frombuffer(raw + b"\0" * (-len(raw) % 8), dtype=np.uint8).view(np.uint64))


# ---- shapes: (setup for amount a, inputs of proof j for amount a)
def shape_2x2(amount):
    rds = [RP.make_range_data(16, 0, 2**64, False, o, False) for o in (False, False, True, True)]
    pts = RP.basis_points(b"public amounts bench", 2 + 6 + 4 + 64 + 8)
    return RP.setup(backend, pts, True, [(True, 0, amount)], rds, "NL")


def inputs_2x2(fee, j, rng):
    total = fee + int(rng.integers(2**40, 2**41))
    i1 = int(rng.integers(0, total)); o1 = int(rng.integers(0, total - fee))
    return [(i1, 0, int(rng.integers(1, 2**63))), (total - i1, 0, int(rng.integers(1, 2**63))), (o1, 0, int(rng.integers(1, 2**63))),
            (total - fee - o1, 0, int(rng.integers(1, 2**63)))]


SCHEMA_128 = dict(json.load(open(os.path.join(EX, "128by64", "schema.json"))), typed=True)
POINTS_128 = RP.basis_points(b"test points", 4 + 1152 + 261 + 8)


def shape_128(amount):
    return RP.setup_from_schema(backend, dict(SCHEMA_128, public=[{"amount": amount, "type": 0}]), POINTS_128)


def inputs_128(pub, j, rng):
    d = [int(x) for x in rng.integers(-5000, 5000, size=64)]
    vals = [pub // 128 + x for x in d] + [pub // 128 - x for x in d]
    vals[0] += pub - sum(vals)                          # the outputs add up to this proof's public input
    return [(v, 0, int(bl)) for v, bl in zip(vals, rng.integers(1, 2**63, size=128, dtype=np.uint64))]


def make_proofs(nat, inputs_fn, amounts, tag, pub):
    rng = np.random.default_rng(zlib.crc32(tag))
    ins = [inputs_fn(a, j, rng) for j, a in enumerate(amounts)]
    pre = [b"%s %06d" % (tag, j) for j in range(len(amounts))]
    files = nat.prove_batch(ins, pre, public_amounts=[[a] for a in amounts] if pub else None)
    return [c for c, _ in files], [p for _, p in files]


result = {"batch": B, "verify": {}, "mixed": {}, "prove": {}}
shapes = [("2x2by64", shape_2x2, inputs_2x2, 1000, 1)] + ([] if args.skip_128 else [("128by64", shape_128, inputs_128, 128 * 10000, 997)])
for name, shape, inputs_fn, base, step in shapes:
    fixed = RP.NativeRangeProofs(gpu, shape(base))
    amounts = [base + step * j for j in range(B)]              # B distinct public amounts
    cf0, pf0 = make_proofs(fixed, inputs_fn, [base] * B, name.encode() + b" fixed", False)
    cf1, pf1 = make_proofs(fixed, inputs_fn, amounts, name.encode() + b" pub", True)
    dc0, dp0, dc1, dp1 = up(cf0), up(pf0), up(cf1), up(pf1)
    d_amt = gpu.to_device(scalars_to_array(amounts))
    routes = {"verify_batch_device (one amount)": lambda: fixed.verify_batch_device(B, dc0, dp0, SEED),
              "verify_batch_pub_device (%d amounts)" % B: lambda: fixed.verify_batch_device(B, dc1, dp1, SEED, public_amounts=d_amt)}
    result["verify"][name] = alternate(routes, args.reps, args.warmup)
    # ---- leg 2: one handle per distinct amount, verify_mixed over them (same proofs, amounts rounded into k groups)
    if name == "2x2by64":
        for k in (16, 64):
            per = B // k
            t0 = time.perf_counter()
            handles = [RP.NativeRangeProofs(gpu, shape(amounts[g * per])) for g in range(k)]
            create_ms = (time.perf_counter() - t0) * 1e3
            grp_amounts = [amounts[(j // per) * per] for j in range(B)]
            cf2, pf2 = make_proofs(fixed, inputs_fn, grp_amounts, b"mixed %d" % k, True)
            dc2, dp2 = up(cf2), up(pf2)
            cb, pb = fixed.shape["coms_bytes"], fixed.shape["proof_bytes"]
            groups = [(handles[g], per, dc2 + g * per * cb, dp2 + g * per * pb) for g in range(k)]
            d_amt2 = gpu.to_device(scalars_to_array(grp_amounts))
            routes = {"verify_mixed_device (%d handles)" % k: lambda: RP.verify_mixed_device(gpu, groups, SEED)[0],
                      "verify_batch_pub_device": lambda: fixed.verify_batch_device(B, dc2, dp2, SEED, public_amounts=d_amt2)}
            r = alternate(routes, args.reps, args.warmup)
            r["handle_creation_ms"] = round(create_ms, 1)
            result["mixed"]["%d amounts" % k] = r
            for h in handles:
                h.close()
            for p in (dc2, dp2, d_amt2):
                gpu.free(p)
    # ---- leg 3: the prover
    if name == "2x2by64":
        rng = np.random.default_rng(3)
        ins0 = [inputs_2x2(base, j, rng) for j in range(B)]
        ins1 = [inputs_2x2(a, j, rng) for j, a in enumerate(amounts)]
        pre = [b"prove %06d" % j for j in range(B)]
        pubs = [[a] for a in amounts]
        routes = {"prove_batch (one amount)": lambda: fixed.prove_batch(ins0, pre),
                  "prove_batch_pub (%d amounts)" % B: lambda: fixed.prove_batch(ins1, pre, public_amounts=pubs)}
        result["prove"][name] = alternate(routes, args.prove_reps, 1)
    for p in (dc0, dp0, dc1, dp1, d_amt):
        gpu.free(p)
    fixed.close()
print(json.dumps(result))
