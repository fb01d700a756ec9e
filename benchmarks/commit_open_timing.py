"""bppp_rp_commit_batch_device and the two ways of checking openings, on one 64by64 handle, device buffers uploaded once outside the timed
region, the legs of a step alternated call by call in one process after a warm-up:

  commit   (a) bppp_rp_commit_batch_device at --batch rows against (b) bppp_rp_prove_batch_device on the same handle and rows — proving is
           the only way the library gave a caller these bytes before the commit entry point existed
  open N   bppp_rp_open_each_device against bppp_rp_open_batch_device at N = 256, 4096 and 65536 rows (--open-rows), every opening true

Without --step this script is the driver: every step runs as a child process of its own under `timeout` (a step that hangs or faults ends
there and nothing is started after it), and the steps' results are printed as one JSON line.  Wall time of the C call only; median, min
and max over --reps timed calls per leg.
   python benchmarks/commit_open_timing.py [--batch 4096] [--open-rows 256,4096,65536] [--reps 20] [--warmup 3] [--step-timeout 600]"""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--open-rows", default="256,4096,65536")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--step-timeout", type=int, default=600)
ap.add_argument("--step", default=None, help="internal: 'commit' or 'open:<rows>'")
args = ap.parse_args()

if args.step is None:
    steps = (["commit"] if args.batch else []) + ["open:%d" % int(n) for n in args.open_rows.split(",") if n.strip()]
    result = {"reps": args.reps, "warmup": args.warmup}
    for step in steps:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--batch", str(args.batch), "--reps", str(args.reps),
               "--warmup", str(args.warmup)]
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
NR, CB, PB = 64, nat.shape["coms_bytes"], nat.shape["proof_bytes"]


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def claims(B):
    """B rows of in-range amounts, zero types and blindings below 2^63, as [B * 64][4] word arrays in HBM"""
    rng = np.random.default_rng(0xC0)
    amt, typ, bld = (np.zeros((B * NR, 4), dtype=np.uint64) for _ in range(3))
    amt[:, 0] = rng.integers(0, 2**63, size=B * NR, dtype=np.uint64) * 2 + rng.integers(0, 2, size=B * NR, dtype=np.uint64)
    bld[:, 0] = rng.integers(1, 2**63, size=B * NR, dtype=np.uint64)
    return [gpu.to_device(a) for a in (amt, typ, bld)]


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


if args.step == "commit":
    B = args.batch
    d_amt, d_typ, d_bld = claims(B)
    pre = np.frombuffer(b"".join(b"commit timing %07d" % i for i in range(B)), dtype=np.uint8)
    plen = len(pre) // B
    d_pre, d_cf, d_cf2, d_pf = gpu.to_device(pre), gpu.alloc(B * CB + 16), gpu.alloc(B * CB + 16), gpu.alloc(B * PB + 16)
    out = run({"commit": lambda: lib.bppp_rp_commit_batch_device(nat.h, B, vp(d_amt), vp(d_typ), vp(d_bld), None, vp(d_cf)),
               "prove": lambda: lib.bppp_rp_prove_batch_device(nat.h, B, vp(d_amt), vp(d_typ), vp(d_bld), None, vp(d_pre), plen, vp(d_cf2), vp(d_pf))})
    same = bool((gpu.download(d_cf, (B * CB,), np.uint8) == gpu.download(d_cf2, (B * CB,), np.uint8)).all())
    print(json.dumps({"rows": B, "ms": out, "same_bytes_as_prover": same, "comb": nat.comb_info()}))
    sys.exit(0 if same else 1)

B = int(args.step.split(":")[1])
d_amt, d_typ, d_bld = claims(B)
d_cf = gpu.alloc(B * CB + 16)
gpu._check(lib.bppp_rp_commit_batch_device(nat.h, B, vp(d_amt), vp(d_typ), vp(d_bld), None, vp(d_cf)), "commit")
status, acc, seed = np.zeros(B * NR, dtype=np.uint32), C.c_int(0), np.frombuffer(os.urandom(32), dtype=np.uint8)
out = run({"open_each": lambda: lib.bppp_rp_open_each_device(nat.h, B, vp(d_cf), vp(d_amt), vp(d_typ), vp(d_bld), vp(status.ctypes.data)),
           "open_batch": lambda: lib.bppp_rp_open_batch_device(nat.h, B, 0, vp(d_cf), vp(d_amt), vp(d_typ), vp(d_bld), vp(seed.ctypes.data), C.byref(acc), None, None)})
ok = acc.value == 1 and not status.any()
print(json.dumps({"rows": B, "ms": out, "all_open": bool(ok)}))
sys.exit(0 if ok else 1)
