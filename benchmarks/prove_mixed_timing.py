"""Proving a job of several setups: one bppp_rp_prove_batch call per handle, every handle over a comb table of its own (--route per_handle:
what the library did before tables could be shared; runs on any commit), against one bppp_rp_prove_mixed call over ONE table per basis
family (--route mixed).  The job is --batch proofs of each of the eight reference examples (tests/golden/examples), all setups over one
getPoints stream ("test points"), default options except comb_min = 1 so that the tables exist from the warm-up on.

Per route, one JSON line: the wall time of the whole job (median, min, max over --reps runs after --warmup runs, ms), the time of each
shape's prove_batch over the table it then has (own table on per_handle, the shared one after mixed; median ms), the window and bytes of
every handle's table, the sum of the distinct tables' bytes and the free HBM before the handles exist and after the last run.

Both routes in one session, each GPU step under its own time limit:
   timeout -k 10 600 python benchmarks/prove_mixed_timing.py --route per_handle && \\
   timeout -k 10 600 python benchmarks/prove_mixed_timing.py --route mixed"""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.getcwd())
import bulletproofspp_amd as b
from bulletproofspp_amd import rangeproof as RP, rangeproof_binary as RB

ap = argparse.ArgumentParser()
ap.add_argument("--route", choices=["per_handle", "mixed"], required=True)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=1)
args = ap.parse_args()
EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "examples")
NAMES = ["32bit", "64bit", "rec_test", "32by64", "64by64", "96by64", "128by64", "bin_test"]
gpu = b.Bppp(0)


def free_hbm():
    """hipMemGetInfo of the runtime the library runs on"""
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


free_start = free_hbm()
backend = RP.GpuBackend(gpu)
points = RP.basis_points(b"test points", 1400)          # the longest prefix any example takes (128by64: 2 + 1284)
jobs = []
for name in NAMES:
    schema = json.load(open(os.path.join(EX, name, "schema.json")))
    wit = json.load(open(os.path.join(EX, name, "witness.json")))
    binary = bool(schema.get("binary", False))
    nat = (RB.NativeBinaryRangeProofs(gpu, RB.setup_from_schema(backend, schema, points)) if binary else
           RP.NativeRangeProofs(gpu, RP.setup_from_schema(backend, schema, points)))
    nat.set_option("comb_min", 1)
    rows = [RP.inputs_from_witness(wit, b"prove mixed %d" % j) for j in range(args.batch)]
    inputs = [[(v, bl) for v, _, bl in r] for r in rows] if binary else rows
    jobs.append((name, nat, inputs, [b"prove mixed rnd %06d" % j for j in range(args.batch)]))


def run_job():
    if args.route == "mixed":
        return RP.prove_mixed(gpu, [(nat, inputs, prefixes) for _, nat, inputs, prefixes in jobs])
    return [nat.prove_batch(inputs, prefixes) for _, nat, inputs, prefixes in jobs]


def timed(f):
    t0 = time.perf_counter()
    f()
    return 1000 * (time.perf_counter() - t0)


for _ in range(args.warmup):
    first = run_job()
whole = [timed(run_job) for _ in range(args.reps)]
per_shape = {name: statistics.median(timed(lambda: nat.prove_batch(inputs, prefixes)) for _ in range(args.reps)) for name, nat, inputs, prefixes in jobs}
tables, distinct = {}, 0.0
for name, nat, _, _ in jobs:
    if hasattr(nat, "comb_info"):
        info = nat.comb_info()
        tables[name] = info
        distinct += info["bytes"] / max(info["users"], 1)
print(json.dumps({"route": args.route, "batch": args.batch, "reps": args.reps, "warmup": args.warmup,
                  "job_ms": {"median": round(statistics.median(whole), 2), "min": round(min(whole), 2), "max": round(max(whole), 2)},
                  "prove_batch_ms": {k: round(v, 2) for k, v in per_shape.items()}, "tables": tables,
                  "distinct_table_bytes": int(distinct) if tables else None,
                  "free_hbm_start": free_start, "free_hbm_end": free_hbm(), "hbm_used_bytes": free_start - free_hbm()}))
for _, nat, _, _ in jobs:
    nat.close()
gpu.close()
