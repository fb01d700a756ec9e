"""The set commitments (bppp_rp_set_*) timed on one 64bit-shaped handle: append, root, paths and verify_paths, each beside the hashlib restatement on
one core and beside a bare upload of the same bytes (bppp_device_alloc + bppp_upload + bppp_device_free: what the host-buffer call cannot go below).

  step append33    2^20 rows of 33 bytes; legs alternated call by call: `empty` (a fresh full store per call, the create and destroy outside the timed
                   region), `onto` (one full store that starts at 2^24 rows - built by appending the same rows 16 times - and keeps growing by the
                   timed appends: its level arrays double during the warm-up calls and not again), `upload` (the bare upload).  Then root () on the
                   large set, and the restatement once.
  step append2056  2^16 rows of 2056 bytes; the same legs, `onto` again a full store of 2^24 rows (256 appends of the same 2^16 rows: 34 GB of
                   uploads before the timed region)
  step paths       a full store of 2^20 rows of 33 bytes; paths for 2^16 random leaves against the upload of the indices plus the download of the paths'
                   size, and set_path_host over prebuilt levels
  step verify      verify_paths for 2^16 and for 2^20 queries (legs alternated) against their uploads, and set_verify_path_host over 2^12 queries, scaled
  step kernels33, kernels2056   `rocprofv3 --kernel-trace --stats` runs of their own; the driver reads every k_rp_set_* kernel's launches and summed time from
                   the stats file and divides the compressions the trace holds (counted here from the shapes: a leaf of r bytes is
                   ceil ((32 + r + 9) / 64), a node 2, a verified path of a 2^20-row set 2 + 2 * 20 + 2) by that time

Without --step this script is the driver: every step runs as a child process of its own under `timeout` (a step that hangs or faults ends there and
nothing is started after it), and the steps' results are printed as one JSON line.  Wall time of the C calls only; median, min and max over --reps
timed calls per leg after --warmup calls.  No pass mark.
   python benchmarks/set_timing.py [--reps 10] [--warmup 2] [--step-timeout 600] [--no-trace]"""
import argparse, ctypes as C, glob, hashlib, json, os, statistics, subprocess, sys, tempfile, time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--step-timeout", type=int, default=600)
ap.add_argument("--no-trace", action="store_true")
ap.add_argument("--step", default=None, help="internal")
args = ap.parse_args()
TRACE_CALLS = 5


def kernel_totals(directory):
    """kernel name -> (calls, total ns) from the kernel stats file of a trace run"""
    import csv
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            if "k_rp_set_" in name:
                short = name[name.index("k_rp_set_"):].split("(")[0].split("E")[0] if name.startswith("_Z") else name[name.index("k_rp_set_"):].split("(")[0]
                calls, total = out.get(short, (0, 0))
                out[short] = (calls + int(row["Calls"]), total + int(row["TotalDurationNs"]))
    return out


if args.step is None:
    result = {"reps": args.reps, "warmup": args.warmup}
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    for step in ("append33", "append2056", "paths", "verify") + (() if args.no_trace else ("kernels33", "kernels2056")):
        cmd = ["timeout", "-k", "10", str(args.step_timeout)]
        tmp = None
        if step.startswith("kernels"):
            tmp = tempfile.mkdtemp(prefix="set_trace_")
            cmd += ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "set", "--"]
        p = subprocess.run(cmd + me + ["--step", step], capture_output=True, text=True)
        if p.returncode:
            result[step] = {"failed": p.returncode, "stderr": p.stderr[-400:]}
            print(json.dumps(result))
            sys.exit(1)                               # nothing more is started on a GPU after a step that failed
        result[step] = json.loads([l for l in p.stdout.strip().splitlines() if l.startswith("{")][-1])
        if tmp:
            comps = result[step].pop("compressions_in_trace")
            kern = {}
            for name, (calls, total) in kernel_totals(tmp).items():
                kern[name] = {"launches": calls, "total_ms": round(total / 1e6, 4)}
                if name in comps:
                    kern[name]["gcompressions_per_s"] = round(comps[name] / (total * 1e-9) / 1e9, 2)
            result[step]["kernels"] = kern
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
TAG = b"set timing"
nat = RP.NativeRangeProofs(gpu, RP.setup_from_schema(RP.GpuBackend(gpu), json.load(open(os.path.join(EX, "64bit", "schema.json")))), oracle_tag=TAG)
rng = np.random.default_rng(0x5E7)


def ok(rc, what):
    if rc:
        raise RuntimeError("%s -> %d (%s)" % (what, rc, lib.bppp_last_error(gpu.h)))


def blob(nbytes):
    return rng.integers(0, 256, size=nbytes, dtype=np.uint8)


def new_set(rb, keep):
    h = vp()
    ok(lib.bppp_rp_set_create(nat.h, rb, keep, C.byref(h)), "create")
    return h


def append(h, arr, rb):
    ok(lib.bppp_rp_set_append(h, arr.size // rb, vp(arr.ctypes.data)), "append")


def upload(arrs, down=0):
    """the bare copies of a host-buffer call: allocate, upload each array, download `down` bytes, free"""
    ptrs = []
    for a in arrs:
        d = vp()
        ok(lib.bppp_device_alloc(gpu.h, a.nbytes, C.byref(d)), "alloc")
        ok(lib.bppp_upload(gpu.h, d, vp(a.ctypes.data), a.nbytes), "upload")
        ptrs.append(d)
    if down:
        d, host = vp(), np.empty(down, dtype=np.uint8)
        ok(lib.bppp_device_alloc(gpu.h, down, C.byref(d)), "alloc")
        ok(lib.bppp_download(gpu.h, vp(host.ctypes.data), d, down), "download")
        ptrs.append(d)
    for d in ptrs:
        ok(lib.bppp_device_free(gpu.h, d), "free")


def timed(legs):
    """legs: name -> (before or None, call); alternated call by call; before () runs outside the timed region and its result is call's argument"""
    times = {k: [] for k in legs}
    for r in range(args.warmup + args.reps):
        for name, (before, call) in legs.items():
            arg = before() if before else None
            t0 = time.perf_counter()
            call(arg)
            dt = (time.perf_counter() - t0) * 1e3
            if r >= args.warmup:
                times[name].append(dt)
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in times.items()}


def append_step(rb, m):
    rows = blob(m * rb)
    big = new_set(rb, 1)
    for _ in range((1 << 24) // m):                   # 2^24 rows, the same m rows again and again: what they hold does not matter to the time
        append(big, rows, rb)
    made = []

    def fresh():
        while made:
            lib.bppp_rp_set_destroy(made.pop())
        made.append(new_set(rb, 1))
        return made[-1]
    out = timed({"empty": (fresh, lambda h: append(h, rows, rb)), "onto": (None, lambda _: append(big, rows, rb)), "upload": (None, lambda _: upload([rows]))})
    root = np.zeros(32, dtype=np.uint8)
    out.update(timed({"root": (None, lambda _: ok(lib.bppp_rp_set_root(big, vp(root.ctypes.data)), "root"))}))
    n = C.c_uint64(0)
    ok(lib.bppp_rp_set_info(big, C.byref(n), None, None, None), "info")
    out["rows_of_the_large_set_at_the_end"] = int(n.value)
    host_rows = [rows[rb * i:rb * i + rb].tobytes() for i in range(m)]
    t0 = time.perf_counter()
    RP.set_root_host(TAG, rb, m, RP.set_peaks_host(TAG, host_rows))
    out["hashlib_one_core_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    out.update({"row_bytes": rb, "rows": m, "bytes": m * rb})
    while made:
        lib.bppp_rp_set_destroy(made.pop())
    lib.bppp_rp_set_destroy(big)
    return out


def set_2p20():
    n, rb = 1 << 20, 33
    rows = blob(n * rb)
    h = new_set(rb, 1)
    append(h, rows, rb)
    root = np.zeros(32, dtype=np.uint8)
    ok(lib.bppp_rp_set_root(h, vp(root.ctypes.data)), "root")
    return n, rb, rows, h, root


def get_paths(h, idx, pb):
    out = np.empty(idx.size * pb, dtype=np.uint8)
    ok(lib.bppp_rp_set_paths(h, idx.size, vp(idx.ctypes.data), vp(out.ctypes.data)), "paths")
    return out


def verify(rb, n, root, idx, rws, pts):
    acc = C.c_int(0)
    ok(lib.bppp_rp_set_verify_paths(nat.h, rb, n, vp(root.ctypes.data), idx.size, vp(idx.ctypes.data), vp(rws.ctypes.data), vp(pts.ctypes.data), None, C.byref(acc)), "verify")
    assert acc.value == 1


def queries(n, rb, rows, h, nq):
    idx = rng.integers(0, n, size=nq, dtype=np.uint64)
    pts = get_paths(h, idx, RP.set_path_bytes(n))
    rws = rows.reshape(n, rb)[idx.astype(np.int64)].reshape(-1).copy()
    return idx, rws, pts


if args.step == "append33":
    res = append_step(33, 1 << 20)
elif args.step == "append2056":
    res = append_step(2056, 1 << 16)
elif args.step == "paths":
    n, rb, rows, h, root = set_2p20()
    nq, pb = 1 << 16, RP.set_path_bytes(n)
    idx = rng.integers(0, n, size=nq, dtype=np.uint64)
    res = timed({"paths": (None, lambda _: get_paths(h, idx, pb)), "upload": (None, lambda _: upload([idx], down=nq * pb))})
    host_rows = [rows[rb * i:rb * i + rb].tobytes() for i in range(n)]
    t0 = time.perf_counter()
    levels = RP.set_levels_host(TAG, host_rows)
    t1 = time.perf_counter()
    host = [RP.set_path_host(TAG, host_rows, int(i), levels) for i in idx[:1 << 12]]
    t2 = time.perf_counter()
    assert b"".join(host) == get_paths(h, idx[:1 << 12].copy(), pb).tobytes()
    res.update({"queries": nq, "path_bytes": pb, "hashlib_levels_ms": round((t1 - t0) * 1e3, 1), "hashlib_paths_ms_scaled_from_4096": round((t2 - t1) * 1e3 * nq / 4096, 1)})
elif args.step == "verify":
    n, rb, rows, h, root = set_2p20()
    small, large = queries(n, rb, rows, h, 1 << 16), queries(n, rb, rows, h, 1 << 20)
    res = timed({"verify_2p16": (None, lambda _: verify(rb, n, root, *small)), "upload_2p16": (None, lambda _: upload(list(small))),
                 "verify_2p20": (None, lambda _: verify(rb, n, root, *large)), "upload_2p20": (None, lambda _: upload(list(large)))})
    pb = RP.set_path_bytes(n)
    t0 = time.perf_counter()
    for q in range(1 << 12):
        assert RP.set_verify_path_host(TAG, rb, n, root.tobytes(), int(small[0][q]), small[1][rb * q:rb * q + rb].tobytes(), small[2][pb * q:pb * q + pb].tobytes()) == 0
    res.update({"hashlib_one_core_ms_per_2p16_scaled_from_4096": round((time.perf_counter() - t0) * 1e3 * 16, 1), "bytes_2p16": sum(a.nbytes for a in small),
                "bytes_2p20": sum(a.nbytes for a in large)})
elif args.step == "kernels33":
    n, rb, rows, h, root = set_2p20()
    lib.bppp_rp_set_destroy(h)
    idx = rws = pts = None
    for c in range(TRACE_CALLS):
        h = new_set(rb, 1)
        append(h, rows, rb)
        if c == 0:
            small, large = queries(n, rb, rows, h, 1 << 16), queries(n, rb, rows, h, 1 << 20)      # two more k_rp_set_paths launches than the timed five
        get_paths(h, small[0], RP.set_path_bytes(n))
        verify(rb, n, root, *large)
        lib.bppp_rp_set_destroy(h)
    # everything the trace holds: 6 appends (set_2p20 () and the five), 7 path calls (two of them the query builders, one over 2^20 leaves), 5 verifications
    res = {"compressions_in_trace": {"k_rp_set_leaf": 6 * n * 2, "k_rp_set_tree": 6 * 2 * (n - 1), "k_rp_set_verify": TRACE_CALLS * (1 << 20) * (2 + 2 * 20 + 2)},
           "note": "6 appends of 2^20 x 33 onto empty; paths for 6 x 2^16 + 2^20 leaves of a 2^20-row set, 20 slots each; 5 verifications of 2^20 paths"}
elif args.step == "kernels2056":
    rb, m = 2056, 1 << 16
    rows = blob(m * rb)
    for c in range(TRACE_CALLS):
        h = new_set(rb, 1)
        append(h, rows, rb)
        lib.bppp_rp_set_destroy(h)
    res = {"compressions_in_trace": {"k_rp_set_leaf": TRACE_CALLS * m * ((32 + rb + 9 + 63) // 64), "k_rp_set_tree": TRACE_CALLS * 2 * (m - 1)},
           "note": "5 appends of 2^16 x 2056 onto empty"}
else:
    raise SystemExit("unknown step")
print(json.dumps(res))
