"""bppp_rp_excess_sign_device, bppp_rp_excess_verify_each_device and bppp_rp_excess_verify_batch_device on one 64by64 handle, against
bppp_rp_tally_each_device and bppp_rp_tally_batch_device over the same pool and CSR job with the blinding revealed, in the same run; device
buffers uploaded once outside the timed region, the legs of a step alternated call by call in one process after a warm-up:

  tx12    2^12 sums of 4 entries each (two inputs, two outputs), the pool as many commitments, every entry its own commitment, the last half
          of each sum subtracted; claims from bppp_rp_tally_claims_device, so every sum is true and every signature valid
  tx16    the same with 2^16 sums
  audit   one sum of 2^20 entries over a pool of as many commitments, all added

Without --step this script is the driver: every step runs as a child process of its own under `timeout` (a step that hangs or faults ends
there and nothing is started after it), and the steps' results are printed as one JSON line.  Wall time of the C call only; median, min
and max over --reps timed calls per leg, and the ratios of the medians to the revealed-blinding tally.  k_rp_excess_mulcheck alone: one more
bppp_rp_excess_verify_each_device call with the handle's TIMING option on, whose HIP-event time is read from its stderr line.
   python benchmarks/excess_timing.py [--steps tx12,tx16,audit] [--reps 10] [--warmup 2] [--step-timeout 600]"""
import argparse, ctypes as C, json, os, re, statistics, subprocess, sys, tempfile, time

SHAPES = {"tx12": (1 << 12, 4), "tx16": (1 << 16, 4), "audit": (1, 1 << 20)}
ap = argparse.ArgumentParser()
ap.add_argument("--steps", default="tx12,tx16,audit")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--step-timeout", type=int, default=600)
ap.add_argument("--step", default=None, help="internal: one of " + ", ".join(SHAPES))
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
NR, CB, SIG = 64, nat.shape["coms_bytes"], RP.EXCESS_SIG_BYTES


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


nsums, per = SHAPES[args.step]
nnz = nsums * per
B = (nnz + NR - 1) // NR                                   # rows of the pool: at least nnz commitments
rng = np.random.default_rng(0x7A)
amt, typ, bld = (np.zeros((B * NR, 4), dtype=np.uint64) for _ in range(3))
amt[:, 0] = rng.integers(0, 2**62, size=B * NR, dtype=np.uint64)
bld[:, 0] = rng.integers(1, 2**63, size=B * NR, dtype=np.uint64)
bld[:, 1] = rng.integers(1, 2**63, size=B * NR, dtype=np.uint64)      # so that no signed sum of four of them is zero
d_amt, d_typ, d_bld = (gpu.to_device(a) for a in (amt, typ, bld))
d_cf = gpu.alloc(B * CB + 16)
gpu._check(lib.bppp_rp_commit_batch_device(nat.h, B, vp(d_amt), vp(d_typ), vp(d_bld), None, vp(d_cf)), "commit")
entries = np.arange(nnz, dtype=np.uint32)
if per == 4:
    entries[(entries % per) >= (per + 1) // 2] |= np.uint32(1 << 31)      # the last half of every sum is subtracted
d_ss, d_en = gpu.to_device(np.arange(nsums + 1, dtype=np.uint32) * np.uint32(per)), gpu.to_device(entries)
d_ca, d_ct, d_cb = (gpu.alloc(nsums * 32 + 16) for _ in range(3))
gpu._check(lib.bppp_rp_tally_claims_device(nat.h, B, vp(d_amt), vp(d_typ), vp(d_bld), nsums, vp(d_ss), vp(d_en), nnz, vp(d_ca), vp(d_ct), vp(d_cb)), "tally_claims")
d_msg, d_sig = gpu.to_device(rng.integers(0, 256, size=nsums * 32, dtype=np.uint8)), gpu.alloc(nsums * SIG + 16)
aux, seed = np.frombuffer(os.urandom(32), dtype=np.uint8), np.frombuffer(os.urandom(32), dtype=np.uint8)
sstat, estat, bstat, tstat = (np.ones(nsums, dtype=np.uint32) for _ in range(4))
acc, tacc = C.c_int(0), C.c_int(0)
sign = lambda: lib.bppp_rp_excess_sign_device(nat.h, nsums, vp(d_cb), vp(d_msg), vp(aux.ctypes.data), vp(d_sig), None, vp(sstat.ctypes.data))
each = lambda: lib.bppp_rp_excess_verify_each_device(nat.h, B, vp(d_cf), nsums, vp(d_ss), vp(d_en), nnz, vp(d_ca), vp(d_ct), vp(d_msg), vp(d_sig), vp(estat.ctypes.data), None)
out = run({"excess_sign": sign,
           "excess_verify_each": each,
           "excess_verify_batch": lambda: lib.bppp_rp_excess_verify_batch_device(nat.h, B, vp(d_cf), nsums, vp(d_ss), vp(d_en), nnz, vp(d_ca), vp(d_ct), vp(d_msg), vp(d_sig), 0,
                                                                                vp(seed.ctypes.data), C.byref(acc), None, None),
           "tally_each": lambda: lib.bppp_rp_tally_each_device(nat.h, B, vp(d_cf), nsums, vp(d_ss), vp(d_en), nnz, vp(d_ca), vp(d_ct), vp(d_cb), vp(tstat.ctypes.data), None),
           "tally_batch": lambda: lib.bppp_rp_tally_batch_device(nat.h, B, vp(d_cf), nsums, vp(d_ss), vp(d_en), nnz, vp(d_ca), vp(d_ct), vp(d_cb), 0, vp(seed.ctypes.data),
                                                                 C.byref(tacc), None, None)})
ok = acc.value == 1 and tacc.value == 1 and not sstat.any() and not estat.any() and not tstat.any()

# k_rp_excess_mulcheck alone: the library's own HIP-event time of one more call, printed on stderr under the TIMING option
sys.stderr.flush()
saved = os.dup(2)
with tempfile.TemporaryFile() as tf:
    os.dup2(tf.fileno(), 2)
    try:
        nat.set_option("timing", 1)
        rc = each()
        nat.set_option("timing", 0)
    finally:
        os.dup2(saved, 2)
        os.close(saved)
    gpu._check(rc, "excess_verify_each (timing)")
    tf.seek(0)
    text = tf.read().decode(errors="replace")
kernel_ms = [float(v) for v in re.findall(r"k_rp_excess_mulcheck\s+\d+ sums\s+([0-9.]+) ms", text)]
ratios = {"verify_each/tally_each": round(out["excess_verify_each"]["median"] / out["tally_each"]["median"], 3),
          "verify_batch/tally_batch": round(out["excess_verify_batch"]["median"] / out["tally_batch"]["median"], 3)}
print(json.dumps({"sums": nsums, "entries": nnz, "pool_commitments": B * NR, "ms": out, "ratios": ratios, "mulcheck_kernel_ms": round(sum(kernel_ms), 3),
                  "mulcheck_launches": len(kernel_ms), "all_true": bool(ok)}))
sys.exit(0 if ok and kernel_ms else 1)
