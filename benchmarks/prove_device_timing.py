"""bppp_rp_prove_batch_device (amounts, types, blindings in HBM -> files in HBM) against bppp_rp_prove_batch_pub (host buffers) on one handle,
the three routes alternated call by call in one process after a warm-up:

  host pageable   bppp_rp_prove_batch_pub from numpy arrays into numpy arrays
  host pinned     the same from and into bppp_host_alloc buffers
  device          bppp_rp_prove_batch_device on device buffers uploaded once, outside the timed region

Shapes: 64by64 (the reference example, norm-linear argument, default comb table) at --batches proofs, and the 64 x 64-bit binary shape of
benchmarks/binary_64by64.py at --binary-batch proofs (0 skips it).  Wall time of the C call only; median, min and max over --reps timed calls
per route.  After the timed calls one call of the host and of the device entry point runs with the TIMING option, whose phase laps (witness,
phases + argument, encode) go to stderr.  Prints one JSON line.
   python benchmarks/prove_device_timing.py [--batches 4096,256] [--binary-batch 1024] [--reps 20] [--warmup 3]"""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import bulletproofspp_amd as b
from bulletproofspp_amd import rangeproof as RP, rangeproof_binary as RB

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="4096,256")
ap.add_argument("--binary-batch", type=int, default=1024)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "examples")
gpu = b.Bppp(0)
lib = gpu.lib
backend = RP.GpuBackend(gpu)
vp = C.c_void_p


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def pinned_copy(a):
    p = gpu.host_alloc(max(a.nbytes, 16))
    p[:a.nbytes] = a.view(np.uint8).reshape(-1)
    return p


def measure(nat, inputs, prefixes, binary):
    """the three routes on one set of inputs: {route: stats}; checks once that all three write the same bytes"""
    B = len(inputs)
    amt, typ, bld, pre, plen, cf, pf = nat._prove_arrays(nat._prove_rows(inputs), prefixes)
    pin = [pinned_copy(a) for a in (amt, typ, bld, pre)]
    pcf, ppf = gpu.host_alloc(cf.nbytes), gpu.host_alloc(pf.nbytes)
    dev = [gpu.to_device(a) for a in (amt, typ, bld, pre)]
    dcf, dpf = gpu.alloc(cf.nbytes + 16), gpu.alloc(pf.nbytes + 16)
    addr = lambda a: vp(a.ctypes.data)

    def host(arrs, ocf, opf):
        return lambda: lib.bppp_rp_prove_batch_pub(nat.h, B, addr(arrs[0]), addr(arrs[1]), addr(arrs[2]), None, addr(arrs[3]), plen, addr(ocf), addr(opf))
    routes = {"host pageable": host((amt, typ, bld, pre), cf, pf), "host pinned": host(pin, pcf, ppf),
              "device": lambda: lib.bppp_rp_prove_batch_device(nat.h, B, vp(dev[0]), vp(0 if binary else dev[1]), vp(dev[2]), None, vp(dev[3]), plen, vp(dcf), vp(dpf))}
    for _ in range(args.warmup):
        for k, fn in routes.items():
            gpu._check(fn(), k)
    assert bytes(cf) == bytes(pcf) == bytes(gpu.download(dcf, cf.shape, np.uint8)) and bytes(pf) == bytes(ppf) == bytes(gpu.download(dpf, pf.shape, np.uint8))
    ms = {k: [] for k in routes}
    for _ in range(args.reps):
        for k, fn in routes.items():
            t = time.perf_counter()
            rc = fn()
            ms[k].append((time.perf_counter() - t) * 1e3)
            gpu._check(rc, k)
    nat.set_option("timing", 1)
    for k in ("host pinned", "device"):
        print("[timing] %s, %d proofs" % (k, B), file=sys.stderr, flush=True)
        gpu._check(routes[k](), k)
    nat.set_option("timing", 0)
    for a in pin + [pcf, ppf]:
        gpu.host_free(a)
    for p in dev + [dcf, dpf]:
        gpu.free(p)
    return {k: stats(v) for k, v in ms.items()}


result = {"reps": args.reps, "warmup": args.warmup}
rng = np.random.default_rng(0xD0)
batches = [int(x) for x in args.batches.split(",") if x]
if batches:
    schema = json.load(open(os.path.join(EX, "64by64", "schema.json")))
    nat = RP.NativeRangeProofs(gpu, RP.setup_from_schema(backend, schema))
    result["64by64"] = {}
    for B in batches:                                   # largest first: the first batch of at least COMB_MIN proofs builds the table
        vals = rng.integers(0, 2**63, size=(B, 64), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(B, 64), dtype=np.uint64)
        bld = rng.integers(1, 2**63, size=(B, 64), dtype=np.uint64)
        inputs = [[(int(v), 0, int(x)) for v, x in zip(vals[i], bld[i])] for i in range(B)]
        result["64by64"][str(B)] = measure(nat, inputs, [b"prove device %08d" % i for i in range(B)], False)
    result["64by64"]["comb"] = nat.comb_info()
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
    result["binary 64x64"] = {str(B): measure(nat, inputs, [b"prove device bin %08d" % i for i in range(B)], True), "comb": nat.comb_info()}
    nat.close()
print(json.dumps(result))
