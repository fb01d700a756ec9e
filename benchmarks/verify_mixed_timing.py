"""bppp_rp_verify_mixed_device (one call, one combined MSM over every setup of the job) against the per-handle calls it replaces (one
bppp_rp_verify_batch_device per setup, in a row), on the same device-resident files, alternated within one process after a warm-up.

  block mix:    256 proofs each of 32by64, 64by64, 96by64, 128by64 (norm-linear), 1024 of 64bit (inner-product), 64 of the 64 x 64-bit
                binary shape (norm-linear, conserved)
  latency mix:  8 proofs of each of the 8 reference examples (tests/golden/examples)

Every setup's basis comes from ONE getPoints stream over "test points" (rangeproof.basis_points), as the reference CLI derives it, so
every handle is one basis family and the mixed call merges their shared terms.  Proofs are made on the GPU by the library's prover with
comb_budget 0 (no fixed-base comb tables piling up in HBM across handles).  Prints one JSON line: per mix the wall time of each route
(median, quartiles, min, max over the repetitions, ms), the ratio of the medians and the MSM term counts.
   python benchmarks/verify_mixed_timing.py [--reps N] [--warmup W]"""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import bulletproofspp_amd as b
from bulletproofspp_amd import rangeproof as RP, rangeproof_binary as RB
from bulletproofspp_amd.capi import load_test_library

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "examples")
NAMES = ["32bit", "64bit", "rec_test", "32by64", "64by64", "96by64", "128by64", "bin_test"]
gpu = b.Bppp(0)
tlib = load_test_library()
backend = RP.GpuBackend(gpu)
points = RP.basis_points(b"test points", 4 + 64 * 64 + 8)          # the longest prefix any setup below takes (binary 64 x 64-bit: 4 + 4096)


def example(name):
    schema = json.load(open(os.path.join(EX, name, "schema.json")))
    wit = json.load(open(os.path.join(EX, name, "witness.json")))
    if schema.get("binary", False):
        nat = RB.NativeBinaryRangeProofs(gpu, RB.setup_from_schema(backend, schema, points))
        make = lambda j: [(v, bl) for v, _, bl in RP.inputs_from_witness(wit, b"mixed %d" % j)]
    else:
        nat = RP.NativeRangeProofs(gpu, RP.setup_from_schema(backend, schema, points))
        make = lambda j: RP.inputs_from_witness(wit, b"mixed %d" % j)
    return nat, make


def binary64():
    count, amount = 64, 10000
    rds = [RB.make_range_data(0, 2**64, True, False)] * count
    nat = RB.NativeBinaryRangeProofs(gpu, RB.setup(backend, points, True, rds, amount * count, "NL"))
    rng = np.random.default_rng(0xB164)

    def make(j):
        d = [int(x) for x in rng.integers(-5000, 5000, size=count // 2)]
        vals = [amount + x for x in d] + [amount - x for x in d]
        return [(v, int(bl)) for v, bl in zip(vals, rng.integers(1, 2**63, size=count, dtype=np.uint64))]
    return nat, make


handles = {n: example(n) for n in NAMES}
handles["bin64x64"] = binary64()
for nat, _ in handles.values():
    nat.set_option("comb_budget", 0)


def prove(name, B, tag):
    nat, make = handles[name]
    cf, pf = [], []
    for lo in range(0, B, 512):                     # prove batches below 1024 proofs
        n = min(512, B - lo)
        files = nat.prove_batch([make(lo + j) for j in range(n)], [b"%s %s %06d" % (tag, name.encode(), lo + j) for j in range(n)])
        cf += [c for c, _ in files]; pf += [p for _, p in files]
    dev = []
    for bs in (cf, pf):
        raw = b"".join(bs)
        dev.append(gpu.to_device(np.frombuffer(raw + b"\0" * (-len(raw) % 8), dtype=np.uint8).view(np.uint64)))
    return nat, B, dev[0], dev[1]


seed = np.frombuffer(b"\x07" * 32, dtype=np.uint8)
acc = C.c_int(0)


def mixed(groups):
    arr = RP._mixed_groups(groups)
    def run():
        rc = gpu.lib.bppp_rp_verify_mixed_device(C.cast(arr, C.c_void_p), len(groups), 0, C.c_void_p(seed.ctypes.data), C.byref(acc), None, None)
        gpu._check(rc, "bppp_rp_verify_mixed_device")
        assert acc.value == 1, "mixed job rejected"
    return run


def separate(groups):
    def run():
        for nat, B, dc, dp in groups:
            rc = gpu.lib.bppp_rp_verify_batch_device(nat.h, B, C.c_void_p(dc), C.c_void_p(dp), C.c_void_p(seed.ctypes.data), C.byref(acc), None, None, None)
            gpu._check(rc, "bppp_rp_verify_batch_device")
            assert acc.value == 1, "per-handle batch rejected"
    return run


def stats(ts):
    ts = sorted(t * 1e3 for t in ts)
    q = statistics.quantiles(ts, n=4) if len(ts) >= 2 else [ts[0]] * 3
    return {"median": round(statistics.median(ts), 4), "p25": round(q[0], 4), "p75": round(q[2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4)}


def measure(groups):
    runs = {"mixed": mixed(groups), "separate": separate(groups)}
    for _ in range(args.warmup):
        for f in runs.values():
            f()
    ts = {k: [] for k in runs}
    for r in range(args.reps):
        order = ["mixed", "separate"] if r % 2 == 0 else ["separate", "mixed"]      # alternated: drifts hit both routes alike
        for k in order:
            t0 = time.perf_counter(); runs[k](); ts[k].append(time.perf_counter() - t0)
    runs["mixed"]()
    t = C.c_uint64(0)
    tlib.bppp_test_last_mixed_msm_terms(gpu.h, C.byref(t))
    per_handle_terms = sum(1 + nat.shape["lin_len"] + nat.shape["norm_len"] + B * ((2 if isinstance(nat, RB.NativeBinaryRangeProofs) else 4) + nat.shape["nranges"] + 2 * nat.shape["rounds"])
                           for nat, B, _, _ in groups)
    out = {"proofs": sum(B for _, B, _, _ in groups), "groups": len(groups), "mixed_ms": stats(ts["mixed"]), "separate_ms": stats(ts["separate"]),
           "speedup_median": round(statistics.median(ts["separate"]) / statistics.median(ts["mixed"]), 3),
           "msm_terms_mixed": t.value, "msm_terms_per_handle_sum": per_handle_terms}
    for _, _, dc, dp in groups:
        gpu.free(dc); gpu.free(dp)
    return out


block = [prove(n, B, b"block") for n, B in (("32by64", 256), ("64by64", 256), ("96by64", 256), ("128by64", 256), ("64bit", 1024), ("bin64x64", 64))]
res_block = measure(block)
latency = [prove(n, 8, b"latency") for n in NAMES]
res_latency = measure(latency)
print(json.dumps({"bench": "verify_mixed_timing", "what": "wall ms of one bppp_rp_verify_mixed_device call vs one bppp_rp_verify_batch_device per setup "
                  "in a row, same device-resident files, alternated in one process after warm-up; one basis family (getPoints \"test points\")",
                  "reps": args.reps, "warmup": args.warmup, "block_mix": res_block, "latency_mix": res_latency}), flush=True)
for nat, _ in handles.values():
    nat.close()
gpu.close()
