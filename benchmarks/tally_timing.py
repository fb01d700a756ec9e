"""bppp_rp_tally_each_device and bppp_rp_tally_batch_device on one 64by64 handle, against bppp_rp_open_batch_device over the same number of
commitments in the same run as the yardstick; device buffers uploaded once outside the timed region, the legs of a step alternated call by
call in one process after a warm-up:

  tx      --sums sums of --per-sum entries each (2^16 x 4: two inputs, two outputs), the pool --sums * --per-sum commitments, every entry its
          own commitment, the last half of each sum subtracted; claims from bppp_rp_tally_claims_device, so every sum is true
  audit   one sum of --audit entries (2^20) over a pool of as many commitments, all added

Without --step this script is the driver: every step runs as a child process of its own under `timeout` (a step that hangs or faults ends
there and nothing is started after it), and the steps' results are printed as one JSON line.  Wall time of the C call only; median, min
and max over --reps timed calls per leg.
   python benchmarks/tally_timing.py [--sums 65536] [--per-sum 4] [--audit 1048576] [--reps 10] [--warmup 2] [--step-timeout 600]"""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--sums", type=int, default=65536)
ap.add_argument("--per-sum", type=int, default=4)
ap.add_argument("--audit", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--step-timeout", type=int, default=600)
ap.add_argument("--step", default=None, help="internal: 'tx' or 'audit'")
args = ap.parse_args()

if args.step is None:
    steps = (["tx"] if args.sums else []) + (["audit"] if args.audit else [])
    result = {"reps": args.reps, "warmup": args.warmup}
    for step in steps:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--sums", str(args.sums), "--per-sum", str(args.per_sum),
               "--audit", str(args.audit), "--reps", str(args.reps), "--warmup", str(args.warmup)]
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
NR, CB = 64, nat.shape["coms_bytes"]


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


if args.step == "tx":
    nsums, per = args.sums, args.per_sum
else:
    nsums, per = 1, args.audit
nnz = nsums * per
B = (nnz + NR - 1) // NR                                   # rows of the pool: at least nnz commitments
rng = np.random.default_rng(0x7A)
amt, typ, bld = (np.zeros((B * NR, 4), dtype=np.uint64) for _ in range(3))
amt[:, 0] = rng.integers(0, 2**62, size=B * NR, dtype=np.uint64)
bld[:, 0] = rng.integers(1, 2**63, size=B * NR, dtype=np.uint64)
d_amt, d_typ, d_bld = (gpu.to_device(a) for a in (amt, typ, bld))
d_cf = gpu.alloc(B * CB + 16)
gpu._check(lib.bppp_rp_commit_batch_device(nat.h, B, vp(d_amt), vp(d_typ), vp(d_bld), None, vp(d_cf)), "commit")
entries = np.arange(nnz, dtype=np.uint32)
if args.step == "tx":
    entries[(entries % per) >= (per + 1) // 2] |= np.uint32(1 << 31)      # the last half of every sum is subtracted
d_ss, d_en = gpu.to_device(np.arange(nsums + 1, dtype=np.uint32) * np.uint32(per)), gpu.to_device(entries)
d_ca, d_ct, d_cb = (gpu.alloc(nsums * 32 + 16) for _ in range(3))
gpu._check(lib.bppp_rp_tally_claims_device(nat.h, B, vp(d_amt), vp(d_typ), vp(d_bld), nsums, vp(d_ss), vp(d_en), nnz, vp(d_ca), vp(d_ct), vp(d_cb)), "tally_claims")
status, acc, oacc, seed = np.ones(nsums, dtype=np.uint32), C.c_int(0), C.c_int(0), np.frombuffer(os.urandom(32), dtype=np.uint8)
out = run({"tally_batch": lambda: lib.bppp_rp_tally_batch_device(nat.h, B, vp(d_cf), nsums, vp(d_ss), vp(d_en), nnz, vp(d_ca), vp(d_ct), vp(d_cb), 0, vp(seed.ctypes.data),
                                                                C.byref(acc), None, None),
           "tally_each": lambda: lib.bppp_rp_tally_each_device(nat.h, B, vp(d_cf), nsums, vp(d_ss), vp(d_en), nnz, vp(d_ca), vp(d_ct), vp(d_cb), vp(status.ctypes.data), None),
           "open_batch": lambda: lib.bppp_rp_open_batch_device(nat.h, B, 0, vp(d_cf), vp(d_amt), vp(d_typ), vp(d_bld), vp(seed.ctypes.data), C.byref(oacc), None, None)})
ok = acc.value == 1 and oacc.value == 1 and not status.any()
print(json.dumps({"sums": nsums, "entries": nnz, "pool_commitments": B * NR, "ms": out, "all_true": bool(ok)}))
sys.exit(0 if ok else 1)
