"""The first two stages of the bucket MSM (csrc/msm.hip) checked on their own output, not through the final point: k_digits with recode.hip.h, the
counting sort's k_hist / k_count_tiles / k_scan_apply and the three scatters k_scatter, k_scatter_ranges and k_scatter_one_read.  After one
msm_device (or batch, or registered-basis) call with explicit window_bits the stages are read back (bppp_test_last_msm_layout / _copy) and compared
with the digit format restated in test_gpu_msm_reduce_known_logs.Fmt (imported, not copied; msm_stages.recode ties the stored digit and the sign
bit to Fmt.digits):

  digit rows and sign mask   every stored digit - the re-biased narrow windows and the negated unbiased top row included - and every bit of the mask;
  counts and starts          count[fb] = the non-zero digits of that (instance, window, |digit|), start its exclusive prefix sum, start[FB] their number;
  entries                    inside a bucket the entries of chunk ch (term index in [ch * per, (ch + 1) * per)) are one contiguous run, the runs in chunk
                             order - for a registered basis in (window, chunk) order, index = window * table_stride + j - and the multiset of
                             (sign, index) of every run is the expected one; the order inside a run is the scatters' own business (LDS atomics);
  final point                the MSM's result is the oracle's, which keeps the read-back honest.

That is the contract between the three scatters, which csrc/msm.hip states in a comment: the positions k_scatter would use, the order inside a
(bucket, chunk) free.  Before the call under test the same context runs an MSM of `stride` terms (n rounded up to 8), so the padding of every
digit row beyond n holds another call's non-zero digits: counts and entries must not see them.

Nothing about which bucket is filled is assumed: everything is derived from the scalars.  Those are the edge scalars of test_gpu_field_group, the
range-border digits of test_gpu_msm_sort_ranges (restated on the format's window offsets), 0, 1, n - 1, (n +- 1) / 2, 2^255 mod n, one non-zero digit
in each window in turn with either sign, and seeded random ones, shuffled so that they fall into every chunk."""
import functools
import random

import numpy as np
import pytest

import msm_stages as S
import pyoracle as O
from bulletproofspp_amd.capi import points_to_array, scalars_to_array
from test_gpu_field_group import _edge_fr
from test_gpu_msm_reduce_known_logs import HALF, _fmt

pytestmark = pytest.mark.gpu

N = O.N
NBASE = 256


def E(**kw):
    return tuple(sorted((k, str(v)) for k, v in kw.items()))


# name: kind ('msm', 'batch', 'basis'), c, n, batch, shared points, the context's environment, and what the plan must report: the scatter (Q, one_read)
# by the bppp_test_last_* hooks and W, acnt, top, CH, per of the layout (window_layout and plan_sort of csrc/msm_plan.hpp, worked out in the comments)
ROUTES = {
    # balanced widths: ceil(256 / c) windows, the first 256 - W (c - 1) of c bits; one chunk below 16 384 terms, two at 20 011
    "c5 k_scatter": ("msm", 5, 1001, 1, True, (), (0, 0), dict(W=52, acnt=48, top=51, CH=1, per=1008)),
    "c13 k_scatter two chunks": ("msm", 13, 20011, 1, True, (), (0, 0), dict(W=20, acnt=16, top=19, CH=2, per=10008)),
    "c13 k_scatter three forced chunks": ("msm", 13, 4099, 1, True, E(BPPP_HIST_CH=3), (0, 0), dict(W=20, acnt=16, top=19, CH=3, per=1368)),
    # uniform widths, 8 divides 256: 32 rows, the top one unbiased and negated
    "c8 uniform": ("msm", 8, 1001, 1, True, (), (0, 0), dict(W=32, acnt=32, top=31, CH=1, per=1008)),
    # 16-bit windows, 2^15 buckets: BPPP_SORT_RANGES picks the scatter; chunks by the XCD rule (32 CUs x n * 4 / Q bytes over 1 MiB): 2 at Q = 2, 1 at Q = 4
    "c16 Q0 k_scatter": ("msm", 16, 20011, 1, True, E(BPPP_SORT_RANGES=0), (0, 0), dict(W=16, acnt=16, top=15, CH=1, per=20016)),
    "c16 Q2 k_scatter_ranges": ("msm", 16, 20011, 1, True, E(BPPP_SORT_RANGES=2), (2, 0), dict(W=16, acnt=16, top=15, CH=2, per=10008)),
    "c16 Q4 k_scatter_ranges": ("msm", 16, 20011, 1, True, (), (4, 0), dict(W=16, acnt=16, top=15, CH=1, per=20016)),
    # forced chunk counts: 5 (80 workgroups, under one round of the 256 CUs: k_scatter_ranges) and 16 (one whole round: k_scatter_one_read, unless switched off)
    "c16 Q4 five chunks": ("msm", 16, 20011, 1, True, E(BPPP_HIST_CH=5), (4, 0), dict(W=16, acnt=16, top=15, CH=5, per=4008)),
    "c16 Q4 one read": ("msm", 16, 20011, 1, True, E(BPPP_HIST_CH=16), (4, 1), dict(W=16, acnt=16, top=15, CH=16, per=1256)),
    "c16 Q4 one read switched off": ("msm", 16, 20011, 1, True, E(BPPP_HIST_CH=16, BPPP_SCATTER_ONE_READ=0), (4, 0), dict(W=16, acnt=16, top=15, CH=16, per=1256)),
    "c16 Q2 one read": ("msm", 16, 20011, 1, True, E(BPPP_HIST_CH=16, BPPP_SORT_RANGES=2), (2, 1), dict(W=16, acnt=16, top=15, CH=16, per=1256)),
    # 301 terms in 16 chunks of 24: the 13th is partial, the last three are empty
    "c16 Q4 one read small": ("msm", 16, 301, 1, True, E(BPPP_HIST_CH=16), (4, 1), dict(W=16, acnt=16, top=15, CH=16, per=24)),
    # batches: uniform widths; 5 divides 255, so a carry window and no negated row; instance * n is no multiple of 8: the sign bits of a step straddle words
    "batch 5 shared c5": ("batch", 5, 301, 5, True, (), (0, 0), dict(W=52, acnt=52, top=-1, CH=1, per=304)),
    "batch 5 per instance c8 two chunks": ("batch", 8, 303, 5, False, E(BPPP_HIST_CH=2), (0, 0), dict(W=32, acnt=32, top=31, CH=2, per=152)),
    # a registered basis: 256 / c + 1 biased rows, one bucket set per instance for all of them
    "basis c8": ("basis", 8, 301, 1, True, (), (0, 0), dict(W=33, acnt=33, top=-1, CH=1, per=304)),
    "basis c8 batch 3 two chunks": ("basis", 8, 301, 3, True, E(BPPP_HIST_CH=2), (0, 0), dict(W=33, acnt=33, top=-1, CH=2, per=152)),
}


def _scalars(fmt, n, seed):
    rnd = random.Random(seed)
    M = fmt.M
    out = [0, 1, N - 1, HALF, HALF + 1, pow(2, 255, N)] + _edge_fr()
    mags = {1, M}
    for q in (2, 4):
        for k in range(1, q + 1):
            mags |= {k * M // q - 1, k * M // q, k * M // q + 1}
    for w in (0, fmt.W // 2, fmt.W - 1):                             # test_gpu_msm_sort_ranges: the range borders in the low, a middle and the top window
        for m in sorted(mags):
            s = (m << fmt.off[w]) % N
            out += [s, N - s]
    for w in range(fmt.W):                                          # one non-zero digit in window w alone (the extreme one: with the carry it owes)
        for d in (1, (1 << (fmt.cw[w] - 1)) - 1, 1 << (fmt.cw[w] - 1)):
            if d and d << fmt.off[w] <= HALF:
                out += [d << fmt.off[w], N - (d << fmt.off[w])]
    out = [s % N for s in out]
    rnd.shuffle(out)
    out = out[:n - n // 4]                                          # at least a quarter random (a short input takes a sample of the above)
    out += [rnd.randrange(N) for _ in range(n - len(out))]
    rnd.shuffle(out)
    return out


@functools.lru_cache(maxsize=None)
def _inputs(kind, c, n, batch):
    fmt = _fmt(c, batch, kind == "basis")
    rows = tuple(tuple(_scalars(fmt, n, 1000 * c + 10 * n + b)) for b in range(batch))
    return fmt, rows, S.recode(fmt, rows)


@pytest.fixture(scope="module")
def contexts(gpu):
    made = S.make_contexts(gpu, [r[5] for r in ROUTES.values()])
    yield made
    S.close_contexts(made)


@pytest.fixture(scope="module")
def base():
    return O.hash_points(b"msm sort stage", 2 * NBASE)


def _launch(g, kind, c, n, batch, shared, rows, pidx, base_arr):
    sc = scalars_to_array([s for r in rows for s in r])
    pts = np.ascontiguousarray(base_arr[pidx])
    ds, dp = g.to_device(sc), g.to_device(pts)
    try:
        if kind == "msm":
            return [g.msm_device(ds, dp, n, window_bits=c)]
        if kind == "batch":
            return g.msm_batch_device(ds, dp, n, batch, shared_points=shared, window_bits=c)
        basis = g.basis(dp, window_bits=c, device=True, n=n)
        try:
            return basis.msm(ds, n, batch)
        finally:
            basis.close()
    finally:
        g.free(ds); g.free(dp)


@pytest.mark.parametrize("name", list(ROUTES))
def test_sort_stage(contexts, oracle_lib, base, name):
    kind, c, n, batch, shared, env, scatter, want = ROUTES[name]
    g, flat = contexts[env], kind == "basis"
    fmt, rows, (stored, neg) = _inputs(kind, c, n, batch)
    assert (fmt.W, fmt.acnt, fmt.top) == (want["W"], want["acnt"], want["top"]) and n % 2 == 1
    base_arr = points_to_array(base)
    # point i of instance b: base point (i + 7 b) mod 256 of the shared half, or of instance b's own pick
    pidx = np.array([(i + (0 if shared else 7 * b)) % NBASE + (0 if shared or b % 2 == 0 else NBASE) for b in range(1 if shared else batch) for i in range(n)])
    stride = (n + 7) & ~7
    # the call before: `stride` terms, the same rows and stride of the digit buffer, every digit of the future padding non-zero with near certainty
    rnd = random.Random(n)
    _launch(g, kind, c, stride, batch, shared, [[rnd.randrange(1, N) for _ in range(stride)] for _ in range(batch)],
            np.arange((1 if shared else batch) * stride) % NBASE, base_arr)
    got = _launch(g, kind, c, n, batch, shared, rows, pidx, base_arr)
    lay = S.layout(g)
    assert S.hooks(g)[:2] == scatter
    assert {k: lay[k] for k in want} == want
    assert (lay["c"], lay["M"], lay["flat"], lay["batch"], lay["n"], lay["stride"], lay["Q"], lay["one_read"]) == (c, fmt.M, int(flat), batch, n, stride, *scatter)
    assert lay["FB"] == (batch if flat else batch * fmt.W) * fmt.M and lay["table_stride"] == (n if flat else 0)
    CH, per, ts = lay["CH"], lay["per"], lay["table_stride"]

    # ---- digit rows and sign mask
    dig = S.read(g, lay, "digits")
    bad = np.argwhere(dig[:, :n].reshape(batch, fmt.W, n) != stored)
    assert bad.size == 0, f"{len(bad)} stored digits differ, first (instance, window, term) {bad[:5].tolist()}"
    if n < stride:
        assert (dig[:, n:] != fmt.M).any(), "the padding holds no stale digit: the test does not show that it places nothing"
    bits, words = S.read(g, lay, "negmask")
    assert (bits == neg.reshape(-1)).all(), np.flatnonzero(bits != neg.reshape(-1))[:10]
    if batch * n % 64:
        assert int(words[-1]) >> (batch * n % 64) == 0, "sign-mask bits beyond the last scalar"

    # ---- counts and starts
    fb, run, ent = S.entries(fmt, stored, neg, flat, CH, per, ts)
    count = S.read(g, lay, "count")
    want_count = np.bincount(fb, minlength=lay["FB"])
    bad = np.flatnonzero(count != want_count)
    assert bad.size == 0, f"{bad.size} counts differ, first buckets {bad[:5].tolist()}: {count[bad[:5]].tolist()} for {want_count[bad[:5]].tolist()}"
    start = S.read(g, lay, "start")
    assert (start == np.concatenate(([0], np.cumsum(want_count)))).all()
    assert lay["total"] == int(start[-1]) == fb.size == int(np.count_nonzero(stored.astype(np.int64) - fmt.M))

    # ---- entries: the runs of a bucket in chunk order, each the expected multiset
    sorted_ = S.read(g, lay, "sorted")
    ofb, orun, oent = S.observed_runs(sorted_, count, flat, CH, per, ts)
    key = ofb * (fmt.W * CH + 1) + orun
    bad = np.flatnonzero(np.diff(key) < 0)
    assert bad.size == 0, f"{bad.size} places where a bucket's runs are not contiguous in chunk order, first position {bad[:5].tolist()}"
    o = np.lexsort((oent, orun, ofb))
    bad = np.flatnonzero((oent[o] != ent) | (orun[o] != run))
    assert bad.size == 0, f"{bad.size} entries differ, first: bucket {fb[bad[:3]].tolist()} run {run[bad[:3]].tolist()} expected {[hex(x) for x in ent[bad[:3]]]} got {[hex(x) for x in oent[o][bad[:3]]]}"
    # what the case is for
    assert want_count.max() >= 2 and (CH == 1 or len(set(run.tolist())) >= min(CH, -(-n // per)))
    if fmt.top >= 0:
        assert (stored[:, fmt.top, :] != fmt.M).any(), "the negated row holds no digit"

    # ---- the final point
    for b in range(batch):
        p = pidx[(0 if shared else b) * n:][:n]
        assert got[b] == S.collapsed_oracle(oracle_lib, base, rows[b], p), (name, b)


def test_the_read_back_refuses_what_it_cannot_serve(base):
    """no general-pipeline MSM on the context yet, the small route since (it lays the workspace out its own way), a size that is not the array's"""
    import ctypes

    import bulletproofspp_amd as b
    from bulletproofspp_amd.capi import TEST_MSM_COUNT, TestMsmLayout, load_test_library
    lib, rep, buf = load_test_library(), TestMsmLayout(), np.zeros(1 << 12, dtype=np.uint32)
    g = b.Bppp(0)
    try:
        assert lib.bppp_test_last_msm_layout(g.h, ctypes.byref(rep)) != 0
        assert lib.bppp_test_last_msm_copy(g.h, TEST_MSM_COUNT, buf.ctypes.data, 64) != 0
        sc, pts = scalars_to_array(list(range(1, 40))), np.ascontiguousarray(points_to_array(base[:39]))
        ds, dp = g.to_device(sc), g.to_device(pts)
        try:
            want = g.msm_device(ds, dp, 39, window_bits=4)           # 64 windows of 8 buckets
            lay = S.layout(g)
            assert (lay["W"], lay["FB"]) == (64, 512) and S.read(g, lay, "count").sum() == lay["total"]
            for bytes_ in (0, 512 * 4 - 4, 512 * 4 + 4):
                assert lib.bppp_test_last_msm_copy(g.h, TEST_MSM_COUNT, buf.ctypes.data, bytes_) != 0
            assert lib.bppp_test_last_msm_copy(g.h, 7, buf.ctypes.data, 512 * 4) != 0
            assert g.msm_device(ds, dp, 39) == want                 # no window_bits: the small route
            assert lib.bppp_test_last_msm_layout(g.h, ctypes.byref(rep)) != 0
        finally:
            g.free(ds); g.free(dp)
    finally:
        g.close()
