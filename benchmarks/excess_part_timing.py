"""The multi-party excess signer on one 64by64 handle against the calls it stands next to, in the same run; device buffers uploaded once outside
the timed region, the legs of a step alternated call by call in one process after a warm-up:

  verify12  bppp_rp_excess_part_verify_device over 2^12 two-party sums (2^13 parts, one joint walk each) against
            bppp_rp_excess_verify_keys_each_device over the 2^12 combined signatures under their aggregated keys (one walk each; that code is as it
            was before the multi-party calls came)
  verify16  the same with 2^16 sums
  sign12    bppp_rp_excess_part_nonces_device and bppp_rp_excess_part_sign_device over 2^12 sessions against bppp_rp_excess_sign_device over as many sums
  walk12    the joint walk b P + c Q (bppp_test_rp_excess_mul2) against two single walks (bppp_test_rp_excess_mul twice) over 2^12 instances; the
            one addition that would join the two single walks is left out, which favours them, and every hook call ends with one inversion an
            instance, which favours the joint walk

Without --step this script is the driver: every step runs as a child process of its own under `timeout` (a step that hangs or faults ends
there and nothing is started after it), and the steps' results are printed as one JSON line.  Wall time of the C call only; median, min
and max over --reps timed calls per leg, and the ratios of the medians.  No pass mark.
   python benchmarks/excess_part_timing.py [--steps verify12,verify16,sign12,walk12] [--reps 10] [--warmup 2] [--step-timeout 600]"""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time

STEPS = {"verify12": 1 << 12, "verify16": 1 << 16, "sign12": 1 << 12, "walk12": 1 << 12}
ap = argparse.ArgumentParser()
ap.add_argument("--steps", default="verify12,verify16,sign12,walk12")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--step-timeout", type=int, default=600)
ap.add_argument("--step", default=None, help="internal: one of " + ", ".join(STEPS))
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
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP

EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "examples")
gpu = b.Bppp(0)
lib = gpu.lib
vp = C.c_void_p
nat = RP.NativeRangeProofs(gpu, RP.setup_from_schema(RP.GpuBackend(gpu), json.load(open(os.path.join(EX, "64by64", "schema.json")))))
SIG, KEY, NONCE, PART = RP.EXCESS_SIG_BYTES, RP.EXCESS_KEY_BYTES, RP.EXCESS_PUBNONCE_BYTES, RP.EXCESS_PARTIAL_BYTES


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


def scalars(rng, n):
    a = np.zeros((n, 4), dtype=np.uint64)
    for k in range(3):
        a[:, k] = rng.integers(1, 2**63, size=n, dtype=np.uint64)
    return a


n = STEPS[args.step]
rng = np.random.default_rng(0x9A)
aux = np.frombuffer(os.urandom(32), dtype=np.uint8)

if args.step == "walk12":
    tl = capi.load_test_library()
    full = lambda: rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)                # walked as 256-bit integers: about half the bits set
    d_b, d_c, d_e = gpu.to_device(full()), gpu.to_device(full()), gpu.to_device(scalars(rng, 2 * n))
    d_keys, d_pts, kstat = gpu.alloc(2 * n * KEY + 16), gpu.alloc(2 * n * 64 + 16), np.ones(2 * n, dtype=np.uint32)
    # 2n points of their own: the signer's X = e B, as affine words
    d_msg, d_sig = gpu.to_device(np.zeros(2 * n * 32, dtype=np.uint8)), gpu.alloc(2 * n * SIG + 16)
    xy = np.zeros((2 * n, 8), dtype=np.uint64)
    gpu._check(lib.bppp_rp_excess_sign_device(nat.h, 2 * n, vp(d_e), vp(d_msg), vp(aux.ctypes.data), vp(d_sig), vp(xy.ctypes.data), vp(kstat.ctypes.data)), "excess_sign")
    d_P, d_Q, d_o1, d_o2, d_o3 = gpu.to_device(xy[:n].copy()), gpu.to_device(xy[n:].copy()), gpu.alloc(n * 64), gpu.alloc(n * 64), gpu.alloc(n * 64)

    def two():
        return tl.bppp_test_rp_excess_mul(nat.h, n, vp(d_b), vp(d_P), vp(d_o2)) or tl.bppp_test_rp_excess_mul(nat.h, n, vp(d_c), vp(d_Q), vp(d_o3))
    out = run({"joint_walk": lambda: tl.bppp_test_rp_excess_mul2(nat.h, n, vp(d_b), vp(d_P), vp(d_c), vp(d_Q), vp(d_o1)), "two_walks": two})
    ok = not kstat.any() and gpu.download(d_o1, (n, 8), np.uint64).any()
    print(json.dumps({"instances": n, "ms": out, "ratios": {"joint_walk/two_walks": round(out["joint_walk"]["median"] / out["two_walks"]["median"], 3)}, "all_true": bool(ok)}))
    sys.exit(0 if ok else 1)

if args.step == "sign12":
    d_e, d_msg = gpu.to_device(scalars(rng, n)), gpu.to_device(rng.integers(0, 256, size=n * 32, dtype=np.uint8))
    d_keys, d_pn, d_an, d_ak, d_pt, d_sig = (gpu.alloc(n * w + 16) for w in (KEY, NONCE, NONCE, KEY, PART, SIG))
    st = [np.ones(n, dtype=np.uint32) for _ in range(5)]
    gpu._check(lib.bppp_rp_excess_keys_device(nat.h, n, vp(d_e), vp(d_keys), vp(st[0].ctypes.data)), "excess_keys")
    gpu._check(lib.bppp_rp_excess_part_nonces_device(nat.h, n, vp(d_e), vp(d_msg), vp(aux.ctypes.data), vp(d_pn), vp(st[1].ctypes.data)), "part_nonces")
    d_ps = gpu.to_device(np.arange(n + 1, dtype=np.uint32))                             # one party a sum: the aggregates are its own nonce and key
    gpu._check(lib.bppp_rp_excess_part_aggregate_device(nat.h, n, n, vp(d_ps), vp(d_pn), vp(d_keys), vp(d_an), vp(d_ak), vp(st[2].ctypes.data)), "part_aggregate")
    out = run({"part_nonces": lambda: lib.bppp_rp_excess_part_nonces_device(nat.h, n, vp(d_e), vp(d_msg), vp(aux.ctypes.data), vp(d_pn), vp(st[1].ctypes.data)),
               "part_sign": lambda: lib.bppp_rp_excess_part_sign_device(nat.h, n, vp(d_e), vp(d_msg), vp(aux.ctypes.data), vp(d_an), vp(d_ak), vp(d_pt), vp(st[3].ctypes.data)),
               "excess_sign": lambda: lib.bppp_rp_excess_sign_device(nat.h, n, vp(d_e), vp(d_msg), vp(aux.ctypes.data), vp(d_sig), None, vp(st[4].ctypes.data))})
    ok = not any(s.any() for s in st)
    ratios = {"part_nonces/excess_sign": round(out["part_nonces"]["median"] / out["excess_sign"]["median"], 3),
              "part_sign/excess_sign": round(out["part_sign"]["median"] / out["excess_sign"]["median"], 3)}
    print(json.dumps({"sessions": n, "ms": out, "ratios": ratios, "all_true": bool(ok)}))
    sys.exit(0 if ok else 1)

# n two-party sums: parts 2t and 2t + 1 sign the message of sum t
parts = 2 * n
msgs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
d_e, d_msg, d_pmsg = gpu.to_device(scalars(rng, parts)), gpu.to_device(msgs), gpu.to_device(np.repeat(msgs, 2, axis=0))
d_keys, d_pn, d_pt = (gpu.alloc(parts * w + 16) for w in (KEY, NONCE, PART))
d_an, d_ak, d_sig = (gpu.alloc(n * w + 16) for w in (NONCE, KEY, SIG))
d_ps = gpu.to_device(np.arange(0, parts + 1, 2, dtype=np.uint32))
pst = [np.ones(parts, dtype=np.uint32) for _ in range(4)]
sst = [np.ones(n, dtype=np.uint32) for _ in range(4)]
gpu._check(lib.bppp_rp_excess_keys_device(nat.h, parts, vp(d_e), vp(d_keys), vp(pst[0].ctypes.data)), "excess_keys")
gpu._check(lib.bppp_rp_excess_part_nonces_device(nat.h, parts, vp(d_e), vp(d_pmsg), vp(aux.ctypes.data), vp(d_pn), vp(pst[1].ctypes.data)), "part_nonces")
gpu._check(lib.bppp_rp_excess_part_aggregate_device(nat.h, n, parts, vp(d_ps), vp(d_pn), vp(d_keys), vp(d_an), vp(d_ak), vp(sst[0].ctypes.data)), "part_aggregate")
d_pan = gpu.to_device(np.repeat(gpu.download(d_an, (n, NONCE), np.uint8), 2, axis=0))
d_pak = gpu.to_device(np.repeat(gpu.download(d_ak, (n, KEY), np.uint8), 2, axis=0))
gpu._check(lib.bppp_rp_excess_part_sign_device(nat.h, parts, vp(d_e), vp(d_pmsg), vp(aux.ctypes.data), vp(d_pan), vp(d_pak), vp(d_pt), vp(pst[2].ctypes.data)), "part_sign")
gpu._check(lib.bppp_rp_excess_part_combine_device(nat.h, n, parts, vp(d_ps), vp(d_pn), vp(d_keys), vp(d_pt), vp(d_msg), vp(d_sig), None, vp(sst[1].ctypes.data)), "part_combine")
out = run({"part_verify": lambda: lib.bppp_rp_excess_part_verify_device(nat.h, n, parts, vp(d_ps), vp(d_pn), vp(d_keys), vp(d_pt), vp(d_msg), vp(pst[3].ctypes.data),
                                                                        vp(sst[2].ctypes.data)),
           "verify_keys_each": lambda: lib.bppp_rp_excess_verify_keys_each_device(nat.h, n, vp(d_ak), vp(d_msg), vp(d_sig), vp(sst[3].ctypes.data))})
ok = not any(s.any() for s in pst + sst)
ratios = {"part_verify/verify_keys_each": round(out["part_verify"]["median"] / out["verify_keys_each"]["median"], 3),
          "per walk: (part_verify / parts) / (verify_keys_each / keys)": round(out["part_verify"]["median"] / parts / (out["verify_keys_each"]["median"] / n), 3)}
print(json.dumps({"sums": n, "parts": parts, "keys": n, "ms": out, "ratios": ratios, "all_true": bool(ok)}))
sys.exit(0 if ok else 1)
