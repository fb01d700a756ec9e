"""bppp_rp_cut_through_device on a block-sized job, an adversarial job next to it, and what the step saves a validator.

One 64bit-shaped handle.  The honest job: T transactions of one input and two outputs, a quarter of the outputs spent inside the set through a row of
their own (nnz = 3 T entries, 3 T rows; T = 2^18: 786432 entries), with claims.  The commitments are real (bppp_rp_commit_batch), made once.

  step cut    legs `honest` and `one_identity`, alternated call by call in one process: the honest job, and 2^20 entries that all reference ONE
              identity with alternating signs — the job a block's author would send to make every entry meet in one slot of the table
  step sums   legs `uncut` and `cut`, alternated: bppp_rp_excess_sums_batch_device over the T sums of the job as received against the same call over
              the one sum that cut-through left (zero claims, no keys: the same MSM work as a real block's) — what the step saves a validator

Without --step this script is the driver: every step runs as a child process of its own under `timeout` (a step that hangs or faults ends there and
nothing is started after it), and the steps' results are printed as one JSON line.  Device buffers are uploaded once outside the timed region; wall
time of the C calls only; median, min and max over --reps timed calls per leg after --warmup calls.  No pass mark.
   python benchmarks/cut_through_timing.py [--log2-tx 18] [--log2-adv 20] [--reps 10] [--warmup 2] [--step-timeout 900]"""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--log2-tx", type=int, default=18)
ap.add_argument("--log2-adv", type=int, default=20)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--step-timeout", type=int, default=900)
ap.add_argument("--step", default=None, help="internal: cut or sums")
args = ap.parse_args()

if args.step is None:
    result = {"reps": args.reps, "warmup": args.warmup, "log2_tx": args.log2_tx, "log2_adv": args.log2_adv}
    for step in ("cut", "sums"):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--log2-tx", str(args.log2_tx), "--log2-adv", str(args.log2_adv)]
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
nat = RP.NativeRangeProofs(gpu, RP.setup_from_schema(RP.GpuBackend(gpu), json.load(open(os.path.join(EX, "64bit", "schema.json")))))
cb = nat.shape["coms_bytes"]
rng = np.random.default_rng(0xC07)
SUB = np.uint32(1 << 31)
T = 1 << args.log2_tx


def words(n, bits):
    """n random integers below 2^bits (bits <= 255) as [n][4] words"""
    w = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    for k in range(4):
        lo = 64 * k
        if bits <= lo:
            w[:, k] = 0
        elif bits < lo + 64:
            w[:, k] &= np.uint64((1 << (bits - lo)) - 1)
    return w


def commit(n):
    amt, typ, bld = words(n, 40), np.zeros((n, 4), dtype=np.uint64), words(n, 250)
    out = np.zeros(n * cb, dtype=np.uint8)
    gpu._check(lib.bppp_rp_commit_batch(nat.h, n, vp(amt.ctypes.data), vp(typ.ctypes.data), vp(bld.ctypes.data), None, vp(out.ctypes.data)), "commit_batch")
    return out.reshape(n, cb)


def honest_job():
    """transaction t has rows 3 t (its input), 3 t + 1, 3 t + 2 (its outputs); every second transaction spends output 0 of the transaction T / 2 before
    it (cyclically), so T / 2 of the 2 T outputs are spent inside the set; arrival order is a random permutation of the transactions"""
    own = commit(3 * T)
    pool = own.copy()
    spender = np.arange(0, T, 2)
    pool[3 * spender] = own[3 * ((spender + T // 2 + 1) % T) + 1]
    order = rng.permutation(T).astype(np.uint32)
    entries = np.stack([(3 * order) | SUB, 3 * order + 1, 3 * order + 2], axis=1).reshape(-1).astype(np.uint32)
    start = (3 * np.arange(T + 1)).astype(np.uint32)
    return pool.reshape(-1), start, entries


def one_identity_job(nnz):
    pool = np.tile(commit(1), (2, 1)).reshape(-1)
    entries = (np.arange(nnz, dtype=np.uint32) & 1) * (SUB + np.uint32(1))          # + row 0, - row 1, ...
    return pool, (4 * np.arange(nnz // 4 + 1)).astype(np.uint32), entries.astype(np.uint32)


class Job:
    def __init__(self, pool, start, entries, claims):
        self.rows, self.nsums, self.nnz = pool.size // cb, start.size - 1, entries.size
        self.d = [gpu.to_device(pool), gpu.to_device(start), gpu.to_device(entries)]
        self.d += [gpu.to_device(a) for a in (words(self.nsums, 40), np.zeros((self.nsums, 4), dtype=np.uint64), words(self.nsums, 250))] if claims else [0, 0, 0]
        self.d_new_coms, self.d_new_entries = gpu.alloc(max(pool.size, 16)), gpu.alloc(self.nnz * 4)
        self.bc, self.cnt = np.zeros((3, 4), dtype=np.uint64), capi.RpCutCounts()

    def cut(self):
        d = self.d
        return lib.bppp_rp_cut_through_device(nat.h, self.rows, vp(d[0]), self.nsums, vp(d[1]), vp(d[2]), self.nnz, vp(d[3]), vp(d[4]), vp(d[5]), None, None, vp(self.d_new_coms),
                                              vp(self.d_new_entries), vp(self.bc.ctypes.data) if d[3] else None, C.byref(self.cnt))

    def counts(self):
        return {n: int(getattr(self.cnt, n)) for n, _ in capi.RpCutCounts._fields_}


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


def geometry():
    g = [C.c_uint64() for _ in range(3)]
    capi.load_test_library().bppp_test_rp_cut_through_last(nat.h, *[C.byref(x) for x in g])
    return dict(zip(("slots", "groups", "passes"), (int(x.value) for x in g)))


honest = Job(*honest_job(), claims=True)
if args.step == "cut":
    adv = Job(*one_identity_job(1 << args.log2_adv), claims=False)
    out = {"ms": run({"honest": honest.cut, "one_identity": adv.cut})}
    gpu._check(honest.cut(), "honest")
    out["honest"] = dict(nnz=honest.nnz, rows=honest.rows, nsums=honest.nsums, **honest.counts(), **geometry())
    gpu._check(adv.cut(), "one_identity")
    out["one_identity"] = dict(nnz=adv.nnz, rows=adv.rows, nsums=adv.nsums, **adv.counts(), **geometry())
    out["ratio one_identity/honest"] = round(out["ms"]["one_identity"]["median"] / out["ms"]["honest"]["median"], 3)
    print(json.dumps(out))
    sys.exit(0)

gpu._check(honest.cut(), "honest")
c = honest.counts()
seed = np.frombuffer(os.urandom(32), dtype=np.uint8)
d_ks_tx, d_ks_blk = gpu.to_device(np.zeros(honest.nsums + 1, dtype=np.uint32)), gpu.to_device(np.zeros(2, dtype=np.uint32))
d_blk_start = gpu.to_device(np.array([0, c["new_nnz"]], dtype=np.uint32))
acc = C.c_int(0)


def uncut():
    d = honest.d
    return lib.bppp_rp_excess_sums_batch_device(nat.h, honest.rows, vp(d[0]), honest.nsums, vp(d[1]), vp(d[2]), honest.nnz, None, None, None, 0, vp(d_ks_tx), None, 0,
                                                vp(seed.ctypes.data), C.byref(acc), None, None)


def cut():
    return lib.bppp_rp_excess_sums_batch_device(nat.h, c["new_rows"], vp(honest.d_new_coms), 1, vp(d_blk_start), vp(honest.d_new_entries), c["new_nnz"], None, None, None, 0,
                                                vp(d_ks_blk), None, 0, vp(seed.ctypes.data), C.byref(acc), None, None)


out = {"ms": run({"uncut": uncut, "cut": cut}), "uncut": dict(rows=honest.rows, nsums=honest.nsums, nnz=honest.nnz), "cut": dict(rows=c["new_rows"], nsums=1, nnz=c["new_nnz"])}
out["ratio cut/uncut"] = round(out["ms"]["cut"]["median"] / out["ms"]["uncut"]["median"], 3)
print(json.dumps(out))
sys.exit(0)
