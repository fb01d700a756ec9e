"""The 16-bit per-chunk histograms of the MSM's counting sort (csrc/msm.hip, MsmPlan::hist16 of csrc/msm_plan.hpp): under a ranged scatter whose
chunks are at most 65535 terms long, k_hist stores a chunk's counts as packed 16-bit values, k_count_tiles16 turns them in place into exclusive
prefixes over the chunks modulo 2^16 (count[] and the tile sums stay 32-bit), and the ranged scatters form a bucket's cursor as start[b] + its
16-bit prefix.  A bucket of 65536 entries or more ("wide") has prefixes that wrapped; the lane that loads its cursor counts the decreases in the
bucket's stored sequence over the chunks before its own and adds 65536 for each.  BPPP_HIST16=0 keeps the 32-bit words; every other plan (k_scatter,
batches, registered bases, a chunk of more than 65535 terms) has no 16-bit form.

Every GPU case forces window_bits = 16 (the only width with a ranged scatter), runs on a context with the default and on one created under
BPPP_HIST16=0, and reads the sort back (msm_stages): count and start are the expected arrays, every (bucket, chunk) run of `sorted` is the expected
multiset at the expected positions (msm_stages.entries / observed_runs), the two contexts agree run for run, and bppp_test_last_hist16 names the
route.  Points are k_i G with k_i = 1 + i mod 16, so the expected point is (sum s_i k_i) G from the logs.

Shapes (256 CUs, 4 bucket ranges): the chunk count is min(32, max(ceil(n / 65536), ceil(32 n / 2^20))) unless BPPP_HIST_CH forces it; 16 chunks are
the fewest that fill a round of CUs and take k_scatter_one_read.
  2^17 uniform            4 chunks (k_scatter_ranges), and 16 forced chunks with BPPP_SCATTER_ONE_READ 1 and 0: no wide bucket
  65535, 65536 equal      2 chunks of 32768: every window has one bucket of 65535 (the largest that is not wide) and of 65536 entries (the smallest wide one)
  150000 equal + 50000    7 chunks of 28576: the wide bucket's prefixes 85728 and 142880 wrap, once each; 4 forced chunks of 50000: the prefixes
                          100000 and 150000 wrap between neighbouring chunks (stored 50000, 34464, 18928); 16 forced chunks: k_scatter_one_read
  70001 equal, 1 chunk    the chunk is longer than 65535: the plan keeps 32-bit words on either context"""
import ctypes
import functools
import random

import numpy as np
import pytest

import msm_stages as S
import pyoracle as O
from bulletproofspp_amd.capi import scalars_to_array
from test_gpu_msm_reduce_known_logs import _fmt

N = O.N
G1 = (O.GX, O.GY)
NLOGS = 16
XCD_CUS, WINDOWS, Q, STEP, AHEAD = 32, 16, 4, 1024 * 8, 4
ENV_KEYS = ("BPPP_SORT_RANGES", "BPPP_SCATTER_ONE_READ", "BPPP_HIST_CH", "BPPP_HIST16", "BPPP_LACC", "BPPP_ACC_SIZED", "BPPP_ACC_FQ29", "BPPP_ACC_FAST")


def E(**kw):
    return tuple(sorted((k, str(v)) for k, v in kw.items()))


# ----------------------------------------------------------------------------- the plan rule, restated (plan_sort of csrc/msm_plan.hpp at c = 16, 256 CUs)
def _plan(n, env):
    env = dict(env)
    ch = min(XCD_CUS, max(1, -(-n // 65536), -(-(XCD_CUS * n) // (1 << 20))))
    ch = int(env.get("BPPP_HIST_CH", ch))
    per = (-(-n // ch) + 7) & ~7
    wgs, cus = WINDOWS * ch, 8 * XCD_CUS
    one = env.get("BPPP_SCATTER_ONE_READ", "1") != "0" and -(-per // STEP) <= AHEAD and wgs >= cus and not 0 < wgs % cus < cus // 4
    h16 = per <= 65535 and env.get("BPPP_HIST16", "1") != "0"
    return dict(CH=ch, per=per, one_read=int(one), hist16=int(h16))


# ----------------------------------------------------------------------------- inputs
def _uniform(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(N) for _ in range(n)]


def _one_scalar(seed):
    """a scalar with a non-zero digit in every 16-bit window: n copies fill one bucket per window"""
    fmt, rnd = _fmt(16, 1, False), random.Random(seed)
    while True:
        s = rnd.randrange(N)
        if all(fmt.digits(s)):
            return s


@functools.lru_cache(maxsize=None)
def _scalars(name):
    if name == "uniform 2^17":
        return tuple(_uniform(1 << 17, 171))
    if name in ("equal 65535", "equal 65536", "equal 70001"):
        return (_one_scalar(17),) * int(name.split()[1])
    assert name == "two wraps"
    return (_one_scalar(18),) * 150000 + tuple(_uniform(50000, 181))


def _recode16(fmt, row):
    """msm_stages.recode for 16 windows of 16 bits (top row 15 negated, K the bias of the others), a scalar's 16 stored digits being the 16-bit words
    of |s| + K: one big-integer addition per scalar, not one loop step per digit.  test_recode16_is_msm_stages_recode ties it to the restated format."""
    assert (fmt.c, fmt.W, fmt.acnt, fmt.top) == (16, 16, 16, 15)
    n = len(row)
    neg = np.fromiter((s > N - s for s in row), dtype=bool, count=n)
    buf = b"".join(((N - s if s > N - s else s) + fmt.K).to_bytes(32, "little") for s in row)
    stored = np.frombuffer(buf, dtype=np.uint16).reshape(n, 16).T.copy()
    stored[15] = np.uint16(fmt.M) - stored[15]
    return stored[None], neg[None]


@functools.lru_cache(maxsize=None)
def _stored(name):
    fmt = _fmt(16, 1, False)
    return fmt, _recode16(fmt, _scalars(name))


@functools.lru_cache(maxsize=None)
def _expected(name, CH, per):
    """count, start and the canonical keys of `sorted` ((bucket, run) << 32 | entry, ascending) by msm_stages.entries"""
    fmt, (stored, neg) = _stored(name)
    fb, run, ent = S.entries(fmt, stored, neg, False, CH, per, 0)
    count = np.bincount(fb, minlength=fmt.W * fmt.M)
    start = np.concatenate(([0], np.cumsum(count)))
    return count, start, _keys(fb, run, ent, CH), _logsum(name)


def _keys(fb, run, ent, CH):
    return ((fb * CH + run).astype(np.uint64) << np.uint64(32)) | ent.astype(np.uint64)


@functools.lru_cache(maxsize=None)
def _logsum(name):
    return sum(s * (1 + i % NLOGS) for i, s in enumerate(_scalars(name))) % N


def _chunk_counts(name, per, CH):
    """[window][chunk][bucket] counts of the non-zero digits, straight from the stored digits"""
    fmt, (stored, _) = _stored(name)
    v = np.abs(stored[0].astype(np.int64) - fmt.M)
    ch = np.arange(v.shape[1]) // per
    return np.stack([np.bincount((ch * fmt.M + v[w] - 1)[v[w] > 0], minlength=CH * fmt.M).reshape(CH, fmt.M) for w in range(fmt.W)])


def _stored_prefixes(cc):
    """what k_count_tiles16 leaves in place of the counts: the exclusive prefix over the chunks modulo 2^16; and the full prefixes"""
    full = np.cumsum(cc, axis=1) - cc
    return (full & 0xFFFF).astype(np.uint16), full


def _recount(st16, total):
    """the scatters' cursor offsets from the stored prefixes alone: the stored value, plus 65536 per decrease of the bucket's stored sequence over
    the chunks 1 .. ch where the bucket's total is 65536 or more"""
    dec = np.zeros(st16.shape, dtype=np.int64)
    dec[:, 1:] = np.cumsum(st16[:, 1:] < st16[:, :-1], axis=1)
    return st16.astype(np.int64) + 65536 * dec * (total >= 65536)[:, None, :]


def _widest_ok(name, window_max, widest):
    """the largest bucket of every window: the equal scalars' own, exactly so where all are equal; the 50000 uniform ones of "two wraps" add a few
    entries to it (2^15 buckets: 1.5 expected), which move no wrap"""
    return (window_max == widest).all() if name.startswith("equal") else ((window_max >= widest) & (window_max < widest + 32)).all()


# name of the scalars, the context's environment, what the case must show: the widest bucket's entries and the chunks after which its stored prefix decreases
CASES = [
    ("uniform 2^17", (), dict(CH=4, per=32768, one_read=0, hist16=1), None, ()),
    ("uniform 2^17", E(BPPP_HIST_CH=16), dict(CH=16, per=8192, one_read=1, hist16=1), None, ()),
    ("uniform 2^17", E(BPPP_HIST_CH=16, BPPP_SCATTER_ONE_READ=0), dict(CH=16, per=8192, one_read=0, hist16=1), None, ()),
    ("equal 65535", (), dict(CH=2, per=32768, one_read=0, hist16=1), 65535, ()),
    ("equal 65536", (), dict(CH=2, per=32768, one_read=0, hist16=1), 65536, ()),
    ("equal 65536", E(BPPP_HIST_CH=16), dict(CH=16, per=4096, one_read=1, hist16=1), 65536, ()),
    ("two wraps", (), dict(CH=7, per=28576, one_read=0, hist16=1), 150000, (2, 4)),
    ("two wraps", E(BPPP_HIST_CH=4), dict(CH=4, per=50000, one_read=0, hist16=1), 150000, (1, 2)),
    ("two wraps", E(BPPP_HIST_CH=16), dict(CH=16, per=12504, one_read=1, hist16=1), 150000, (5, 10)),
    ("equal 70001", E(BPPP_HIST_CH=1), dict(CH=1, per=70008, one_read=0, hist16=0), 70001, ()),
]
IDS = [f"{name}{' ' if env else ''}{' '.join(f'{k[5:]}={v}' for k, v in env)}" for name, env, *_ in CASES]


# ----------------------------------------------------------------------------- CPU-only tests
def test_recode16_is_msm_stages_recode():
    fmt = _fmt(16, 1, False)
    half = (N - 1) // 2
    row = [0, 1, N - 1, half, half + 1, pow(2, 255, N), 1 << 15, (1 << 15) - 1, (1 << 16) - 1, N - (1 << 15), _one_scalar(17)] + _uniform(240, 5)
    stored, neg = _recode16(fmt, row)
    want_stored, want_neg = S.recode(fmt, [row])
    assert (stored == want_stored).all() and (neg == want_neg).all()
    for name in ("equal 65535", "two wraps"):
        assert all(fmt.digits(_scalars(name)[0]))


@pytest.mark.parametrize("name,env,want,widest,wraps", CASES, ids=IDS)
def test_the_plan_and_the_recount_on_the_cases_counts(name, env, want, widest, wraps):
    """the restated plan gives the literals; the case holds what it is for (the widest bucket of every window, the chunks after which its stored prefix
    decreases); and the stored 16-bit prefixes with the decreases counted give back every full prefix, wide bucket or not"""
    n = len(_scalars(name))
    assert _plan(n, env) == want and _plan(n, env + E(BPPP_HIST16=0)) == dict(want, hist16=0)
    cc = _chunk_counts(name, want["per"], want["CH"])
    assert cc.max() <= want["per"]
    total = cc.sum(axis=1)
    if widest is None:
        assert total.max() < 65536 and total.max() >= 2
    else:
        assert _widest_ok(name, total.max(axis=1), widest), "one bucket of that size in every window"
    if want["per"] > 65535:
        return
    st16, full = _stored_prefixes(cc)
    assert (_recount(st16, total) == full).all()
    if widest is not None:
        for w in range(WINDOWS):
            seq = st16[w, :, int(total[w].argmax())].astype(np.int64)
            assert tuple(np.flatnonzero(seq[1:] < seq[:-1]).tolist()) == wraps, (w, seq.tolist())


def test_recount_model_on_wraps_in_a_row():
    """every chunk adds under 65536, so a wrapped prefix is below the one before it and an unwrapped one is not: 65535 per chunk decreases by one each time"""
    cc = np.array([65535, 65535, 0, 65535, 1, 65534, 65535, 0], dtype=np.int64).reshape(1, 8, 1)
    st16, full = _stored_prefixes(cc)
    assert (_recount(st16, cc.sum(axis=1)) == full).all() and full.max() == 5 * 65535


# ----------------------------------------------------------------------------- the GPU side
@pytest.fixture(scope="module")
def contexts():
    """environment -> context created under it (the BPPP_* tuning is read once, at creation), made on first use"""
    import bulletproofspp_amd as b
    made = {}

    def get(env):
        if env not in made:
            with pytest.MonkeyPatch.context() as mp:
                for k in ENV_KEYS:
                    mp.delenv(k, raising=False)
                for k, v in env:
                    mp.setenv(k, v)
                made[env] = b.Bppp(0)
        return made[env]
    yield get
    for g in made.values():
        g.close()


@pytest.fixture(scope="module")
def log_points(oracle_lib):
    """(1 + i mod 16) G for i < n, as the n x 8 uint64 affine array of the C ABI"""
    rows = []
    for k in range(1, NLOGS + 1):
        x, y = oracle_lib.mul(k, G1)
        rows.append(np.frombuffer(x.to_bytes(32, "little") + y.to_bytes(32, "little"), dtype=np.uint64))
    table = np.stack(rows)
    return lambda n: np.ascontiguousarray(table[np.arange(n) % NLOGS])


def _hist16(g):
    from bulletproofspp_amd.capi import load_test_library
    v = ctypes.c_int(-2)
    assert load_test_library().bppp_test_last_hist16(g.h, ctypes.byref(v)) == 0
    return v.value


def _run(g, sc, pts, n):
    ds, dp = g.to_device(sc), g.to_device(pts)
    try:
        point = g.msm_device(ds, dp, n, window_bits=16)
    finally:
        g.free(ds); g.free(dp)
    lay = S.layout(g)
    return point, lay, _hist16(g), S.hooks(g)[:2], S.read(g, lay, "count"), S.read(g, lay, "start"), S.read(g, lay, "sorted")


@pytest.mark.gpu
def test_no_msm_yet_reports_minus_one():
    import bulletproofspp_amd as b
    g = b.Bppp(0)
    try:
        assert _hist16(g) == -1
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,want,widest,wraps", CASES, ids=IDS)
def test_hist16(contexts, oracle_lib, log_points, name, env, want, widest, wraps):
    row = _scalars(name)
    n = len(row)
    count, start, keys, logsum = _expected(name, want["CH"], want["per"])
    want_point = oracle_lib.mul(logsum, G1) if logsum else None
    sc, pts = scalars_to_array(list(row)), log_points(n)
    seen = []
    for off in (False, True):
        g = contexts(env + E(BPPP_HIST16=0) if off else env)
        point, lay, h16, (q, one), got_count, got_start, got_sorted = _run(g, sc, pts, n)
        assert h16 == (0 if off else want["hist16"]) and (q, one) == (Q, want["one_read"])
        assert (lay["c"], lay["W"], lay["M"], lay["n"], lay["CH"], lay["per"], lay["Q"], lay["one_read"]) == (16, WINDOWS, 1 << 15, n, want["CH"], want["per"], Q, want["one_read"])
        bad = np.flatnonzero(got_count != count)
        assert bad.size == 0, f"{bad.size} counts differ, first buckets {bad[:5].tolist()}: {got_count[bad[:5]].tolist()} for {count[bad[:5]].tolist()}"
        assert (got_start == start).all() and lay["total"] == int(start[-1]) == keys.size
        ofb, orun, oent = S.observed_runs(got_sorted, got_count, False, want["CH"], want["per"], 0)
        okeys = _keys(ofb, orun, oent, want["CH"])
        bad = np.flatnonzero(np.diff((okeys >> np.uint64(32)).astype(np.int64)) < 0)
        assert bad.size == 0, f"{bad.size} places where a bucket's runs are not contiguous in chunk order, first position {bad[:5].tolist()}"
        okeys.sort()
        bad = np.flatnonzero(okeys != keys)
        assert bad.size == 0, f"{bad.size} entries differ, first: (bucket * CH + run, entry) {[(int(k >> np.uint64(32)), hex(int(k) & 0xFFFFFFFF)) for k in okeys[bad[:3]]]}"
        assert point == want_point, (name, env, off)
        seen.append((point, got_count, got_start, okeys))
    assert seen[0][0] == seen[1][0] and all((a == b).all() for a, b in zip(seen[0][1:], seen[1][1:])), "BPPP_HIST16=0 against the default"
    if widest is not None:
        assert _widest_ok(name, count.reshape(WINDOWS, -1).max(axis=1), widest)
