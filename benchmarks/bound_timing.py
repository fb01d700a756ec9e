"""The bound entry points (per-proof transcript bindings) against their unbound counterparts on one 64by64 handle, device buffers uploaded and
the proofs made once outside the timed region, the legs of a step alternated call by call in one process after a warm-up:

  verify   (a) bppp_rp_verify_shard_pub_device on --batch unbound proofs against (b) bppp_rp_verify_bound_device on the same witnesses' bound proofs
  prove    (a) bppp_rp_prove_batch_device against (b) bppp_rp_prove_bound_device, same inputs; the bound files must differ from the unbound ones in
           the proofs and agree in the commitments

By construction the bound path adds one header kernel (64 bytes written per hash: 3.9 MB at 4096 proofs x 15 hashes) and a per-lane header read.
--other-lib PATH names another build of libbppp_hip.so (the parent commit's): its unbound legs are timed in steps of their own, alternating with
this build's (this, other, this, other ... --rounds times), so that "unbound, this build" can be read against "unbound, parent" and against the
spread of the parent's own medians.  A build without the bound symbols runs its unbound legs only.

Without --step this script is the driver: every step runs as a child process of its own under `timeout` (a step that hangs or faults ends there
and nothing is started after it), and the steps' results are printed as one JSON line.  Wall time of the C call only; median, min and max over
--reps timed calls per leg.
   python benchmarks/bound_timing.py [--batch 4096] [--reps 20] [--warmup 3] [--rounds 2] [--other-lib PATH] [--step-timeout 600]"""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--other-lib", default=None)
ap.add_argument("--step-timeout", type=int, default=600)
ap.add_argument("--step", default=None, help="internal: 'verify' or 'prove'")
ap.add_argument("--lib", default=None, help="internal: the library this step loads instead of the tree's")
args = ap.parse_args()

if args.step is None:
    result = {"batch": args.batch, "reps": args.reps, "warmup": args.warmup, "steps": []}
    for step in ("verify", "prove"):
        for rnd in range(args.rounds):
            for which, lib in (("this", None), ("other", args.other_lib)):
                if which == "other" and not lib:
                    continue
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--batch", str(args.batch),
                       "--reps", str(args.reps), "--warmup", str(args.warmup)] + (["--lib", lib] if lib else [])
                p = subprocess.run(cmd, capture_output=True, text=True)
                if p.returncode:
                    result["steps"].append({"step": step, "build": which, "failed": p.returncode, "stderr": p.stderr[-400:]})
                    print(json.dumps(result))
                    sys.exit(1)                       # nothing more is started on a GPU after a step that failed
                result["steps"].append(dict(json.loads(p.stdout.strip().splitlines()[-1]), step=step, build=which, round=rnd))
    print(json.dumps(result))
    sys.exit(0)

sys.path.insert(0, os.getcwd())
import numpy as np
from bulletproofspp_amd import capi



class _Absent:                                        # an older build lacks the newest symbols: capi.load_library types them, nothing here calls them
    argtypes = restype = None


if args.lib:
    class _OlderBuild(C.CDLL):
        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                if not name.startswith("bppp_"):
                    raise
                return _Absent()

    capi.lib_path = lambda: args.lib
    capi.C.CDLL = _OlderBuild
import bulletproofspp_amd as b
from bulletproofspp_amd import rangeproof as RP

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "examples")
gpu = b.Bppp(0)
lib = gpu.lib
vp = C.c_void_p
nat = RP.NativeRangeProofs(gpu, RP.setup_from_schema(RP.GpuBackend(gpu), json.load(open(os.path.join(EX, "64by64", "schema.json")))), oracle_tag=b"bound timing")
NR, CB, PB = 64, nat.shape["coms_bytes"], nat.shape["proof_bytes"]
HAS_BOUND = not isinstance(lib.bppp_rp_prove_bound_device, _Absent)
B = args.batch


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


rng = np.random.default_rng(0xB0)
amt, typ, bld = (np.zeros((B * NR, 4), dtype=np.uint64) for _ in range(3))
amt[:, 0] = rng.integers(0, 2**63, size=B * NR, dtype=np.uint64) * 2 + rng.integers(0, 2, size=B * NR, dtype=np.uint64)
bld[:, 0] = rng.integers(1, 2**63, size=B * NR, dtype=np.uint64)
d_amt, d_typ, d_bld = (gpu.to_device(a) for a in (amt, typ, bld))
pre = np.frombuffer(b"".join(b"bound timing %07d" % i for i in range(B)), dtype=np.uint8)
plen = len(pre) // B
d_pre = gpu.to_device(pre)
d_bind = gpu.to_device(rng.integers(0, 256, size=(B, 32), dtype=np.uint8))
d_cf, d_pf, d_cfb, d_pfb = gpu.alloc(B * CB + 16), gpu.alloc(B * PB + 16), gpu.alloc(B * CB + 16), gpu.alloc(B * PB + 16)
prove = {"unbound": lambda: lib.bppp_rp_prove_batch_device(nat.h, B, vp(d_amt), vp(d_typ), vp(d_bld), None, vp(d_pre), plen, vp(d_cf), vp(d_pf))}
if HAS_BOUND:
    prove["bound"] = lambda: lib.bppp_rp_prove_bound_device(nat.h, B, vp(d_amt), vp(d_typ), vp(d_bld), None, vp(d_bind), vp(d_pre), plen, vp(d_cfb), vp(d_pfb), None)
for k, fn in prove.items():                           # the comb table and both sets of files, outside the timed region
    gpu._check(fn(), k)
out = {"rows": B, "has_bound": HAS_BOUND, "comb": nat.comb_info()}
ok = True
if HAS_BOUND:
    same_coms = bool((gpu.download(d_cf, (B * CB,), np.uint8) == gpu.download(d_cfb, (B * CB,), np.uint8)).all())
    other_proofs = bool((gpu.download(d_pf, (B * PB,), np.uint8).reshape(B, PB) != gpu.download(d_pfb, (B * PB,), np.uint8).reshape(B, PB)).any(axis=1).all())
    out.update(same_commitments=same_coms, every_proof_differs=other_proofs)
    ok = same_coms and other_proofs
if args.step == "prove":
    out["ms"] = run(prove)
else:
    seed, acc_u, acc_b = np.frombuffer(os.urandom(32), dtype=np.uint8), C.c_int(0), C.c_int(0)
    verify = {"unbound": lambda: lib.bppp_rp_verify_shard_pub_device(nat.h, B, 0, vp(d_cf), vp(d_pf), None, vp(seed.ctypes.data), C.byref(acc_u), None, None, None)}
    if HAS_BOUND:
        verify["bound"] = lambda: lib.bppp_rp_verify_bound_device(nat.h, B, 0, vp(d_cfb), vp(d_pfb), None, vp(d_bind), vp(seed.ctypes.data), C.byref(acc_b), None, None, None)
    out["ms"] = run(verify)
    ok = ok and acc_u.value == 1 and (not HAS_BOUND or acc_b.value == 1)
    out["accepted"] = [acc_u.value, acc_b.value if HAS_BOUND else None]
print(json.dumps(out))
sys.exit(0 if ok else 1)
