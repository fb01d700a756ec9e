"""bppp_rp_prove_batch_status_device (a verdict per proof, the refused proofs skipped) against bppp_rp_prove_batch_device on one handle, device
buffers uploaded once outside the timed region, the legs alternated call by call in one process after a warm-up:

  device              (a) bppp_rp_prove_batch_device, every witness good
  status 0            (b) bppp_rp_prove_batch_status_device on the same inputs: the same kernels
  status 1 / 64 / half (c) ... with 1, 64 and half of the proofs refused (an amount at its range's maximum, spread evenly over the batch)
  device half         bppp_rp_prove_batch_device on half as many proofs: what "half refused" should come close to

Shapes: 64by64 (the reference example, norm-linear argument, default comb table) at --batch proofs, and the 64 x 64-bit binary shape of
benchmarks/binary_64by64.py at --binary-batch proofs (0 skips either).  Wall time of the C call only; median, min and max over --reps timed
calls per leg.  On a library without the status entry points (the parent commit) only the `device` legs run: the same script, the same
session, shows whether the existing entry point moved.  Prints one JSON line.
   python benchmarks/prove_status_timing.py [--batch 4096] [--binary-batch 1024] [--reps 20] [--warmup 3]"""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import bulletproofspp_amd as b
from bulletproofspp_amd import capi, rangeproof as RP, rangeproof_binary as RB

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--binary-batch", type=int, default=1024)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "examples")
gpu = b.Bppp(0)
lib = gpu.lib
backend = RP.GpuBackend(gpu)
vp = C.c_void_p
HAS_STATUS = hasattr(lib, "bppp_rp_prove_batch_status_device")
if HAS_STATUS:
    lib.bppp_rp_prove_batch_status_device.argtypes = [vp, C.c_size_t, vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp]


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def measure(nat, inputs, prefixes, binary):
    B = len(inputs)
    amt, typ, bld, pre, plen, cf, pf = nat._prove_arrays(nat._prove_rows(inputs), prefixes)
    nr = amt.shape[0] // B
    hi = capi.int_to_limbs(2**64)                                   # every range of both shapes is [0, 2^64)
    d_typ, d_bld, d_pre = (gpu.to_device(a) for a in (typ, bld, pre))
    dcf, dpf = gpu.alloc(cf.nbytes + 16), gpu.alloc(pf.nbytes + 16)
    held = [d_typ, d_bld, d_pre, dcf, dpf]
    status = np.zeros(B, dtype=np.uint32)

    def amounts(refused):
        a = amt.copy()
        for j in range(refused):
            a[(j * B // refused) * nr + j % nr] = hi
        held.append(gpu.to_device(a))
        return held[-1]

    def plain(n, d_amt):
        return lambda: lib.bppp_rp_prove_batch_device(nat.h, n, vp(d_amt), vp(0 if binary else d_typ), vp(d_bld), None, vp(d_pre), plen, vp(dcf), vp(dpf))

    def with_status(d_amt):
        return lambda: lib.bppp_rp_prove_batch_status_device(nat.h, B, vp(d_amt), vp(0 if binary else d_typ), vp(d_bld), None, vp(d_pre), plen, vp(dcf), vp(dpf),
                                                             vp(status.ctypes.data))
    good = amounts(0)
    legs, want = {"device": plain(B, good)}, {"device": 0}
    if HAS_STATUS:
        for refused in (0, 1, 64, B // 2):
            if refused <= B:
                name = "status half" if refused == B // 2 else "status %d" % refused
                legs[name], want[name] = with_status(amounts(refused)), refused
    legs["device half"], want["device half"] = plain(B // 2, good), 0
    for _ in range(args.warmup):
        for k, fn in legs.items():
            gpu._check(fn(), k)
            if k.startswith("status"):
                assert int(np.count_nonzero(status)) == want[k], (k, int(np.count_nonzero(status)))
    ms = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            t = time.perf_counter()
            rc = fn()
            ms[k].append((time.perf_counter() - t) * 1e3)
            gpu._check(rc, k)
    for p in held:
        gpu.free(p)
    return {k: stats(v) for k, v in ms.items()}


result = {"reps": args.reps, "warmup": args.warmup, "status_entry_points": HAS_STATUS}
rng = np.random.default_rng(0xD0)
if args.batch:
    B = args.batch
    schema = json.load(open(os.path.join(EX, "64by64", "schema.json")))
    nat = RP.NativeRangeProofs(gpu, RP.setup_from_schema(backend, schema))
    vals = rng.integers(0, 2**63, size=(B, 64), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(B, 64), dtype=np.uint64)
    bld = rng.integers(1, 2**63, size=(B, 64), dtype=np.uint64)
    inputs = [[(int(v), 0, int(x)) for v, x in zip(vals[i], bld[i])] for i in range(B)]
    result["64by64"] = {str(B): measure(nat, inputs, [b"prove status %08d" % i for i in range(B)], False), "comb": nat.comb_info()}
    nat.close()
if args.binary_batch:
    B, count, amount = args.binary_batch, 64, 10000
    rds = [RB.make_range_data(0, 2**64, True, False)] * count
    pts = RP.basis_points(b"prove device binary", 4 + sum(len(rd.base_coeffs) for rd in rds))
    nat = RB.NativeBinaryRangeProofs(gpu, RB.setup(backend, pts, True, rds, amount * count, "NL"), h=pts[0])
    nat.set_option("comb_min", min(B, 1024))
    dlt = rng.integers(-5000, 5000, size=(B, count // 2))
    vals = np.concatenate([amount + dlt, amount - dlt], axis=1).astype(np.uint64)
    bld = rng.integers(1, 2**63, size=(B, count), dtype=np.uint64)
    inputs = [[(int(v), int(x)) for v, x in zip(vals[i], bld[i])] for i in range(B)]
    result["binary 64x64"] = {str(B): measure(nat, inputs, [b"prove status bin %08d" % i for i in range(B)], True), "comb": nat.comb_info()}
    nat.close()
print(json.dumps(result))
