"""Accumulation of whole buckets in order of size (k_order, k_acc_points_sized, k_merge_heavy<true>; BPPP_ACC_SIZED, read when a context is
created): one MSM over arbitrary points gives every lane one bucket, or one piece of at most CAP = 128 entries of a larger bucket.  A context
with BPPP_ACC_SIZED=1 runs beside one with BPPP_ACC_SIZED=0 (the slices of k_acc_points / k_merge); both report their route through
bppp_test_last_acc_sized.  window_bits is passed so that small inputs take the general pipeline with wide windows.  Up to 2^13 terms the
expected value is the oracle's (oracle/pyoracle.py); above, the =0 context's and an oracle value of an equivalent short sum."""
import ctypes
import os
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd.capi import int_to_limbs, limbs_to_int, points_to_array, scalars_to_array

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)
CAP = 128                         # ACC_CAP of csrc/msm.hip
WINDOWS = (16, 13, 8)
SIZES = (1, 63, 64, 65, 1000, 1 << 13)


def _oracle(ec, sc, pts):
    sc, pts = np.ascontiguousarray(sc), np.ascontiguousarray(pts)
    return ec.inner_product_raw(sc.ctypes.data_as(U64P), pts.ctypes.data_as(U64P), sc.shape[0])


@pytest.fixture(scope="module")
def ctxs():
    """[sized, slices]: the environment is read at creation and restored afterwards"""
    import bulletproofspp_amd as b
    old = os.environ.get("BPPP_ACC_SIZED")
    out = []
    try:
        for v in ("1", "0"):
            os.environ["BPPP_ACC_SIZED"] = v
            out.append(b.Bppp(0))
    finally:
        if old is None:
            os.environ.pop("BPPP_ACC_SIZED", None)
        else:
            os.environ["BPPP_ACC_SIZED"] = old
    yield out
    for g in out:
        g.close()


@pytest.fixture(scope="module")
def base_points():
    return points_to_array(O.hash_points(b"acc sized", 1 << 13))


def _last_sized(g):
    from bulletproofspp_amd.capi import load_test_library
    v = ctypes.c_int(-2)
    assert load_test_library().bppp_test_last_acc_sized(g.h, ctypes.byref(v)) == 0
    return v.value


def _run(ctxs, sc_arr, pt_arr, c):
    """the MSM on both contexts; each reports the route it was created for.  Returns the sized result after comparing the two."""
    n = sc_arr.shape[0]
    out = []
    for want, g in zip((1, 0), ctxs):
        ds, dp = g.to_device(sc_arr), g.to_device(pt_arr)
        try:
            out.append(g.msm_device(ds, dp, n, window_bits=c))
        finally:
            g.free(ds); g.free(dp)
        assert _last_sized(g) == want, (want, _last_sized(g))
    assert out[0] == out[1], ("sized != slices", c, n)
    return out[0]


# ---- window and size sweep: fewer items than a wavefront, ragged last wavefronts, classes of size 1
@pytest.fixture(scope="module")
def sweep_cases(oracle_lib, base_points):
    rnd = random.Random(41)
    cases = {}
    for n in SIZES:
        sc = scalars_to_array([rnd.randrange(O.N) for _ in range(n)])
        pts = np.ascontiguousarray(base_points[:n])
        cases[n] = (sc, pts, _oracle(oracle_lib, sc, pts))
    return cases


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("c", WINDOWS)
def test_window_and_size_sweep(ctxs, sweep_cases, c, n):
    sc, pts, want = sweep_cases[n]
    assert _run(ctxs, sc, pts, c) == want


# ---- heavy buckets
@pytest.mark.parametrize("c", WINDOWS)
def test_one_heavy_bucket(ctxs, oracle_lib, base_points, c):
    """all scalars equal at n = 3 CAP + 5: one bucket of 4 pieces in every window, the last piece 5 entries long"""
    n = 3 * CAP + 5
    rnd = random.Random(42)
    sc = scalars_to_array([rnd.randrange(O.N)] * n)
    pts = np.ascontiguousarray(base_points[:n])
    assert _run(ctxs, sc, pts, c) == _oracle(oracle_lib, sc, pts)


@pytest.mark.parametrize("n", (1 << 15, (1 << 15) + 1))
def test_many_pieces(ctxs, oracle_lib, base_points, n):
    """2^15 equal scalars at 16-bit windows: one bucket of 256 pieces per window, a full chunk of k_merge_heavy; one entry more makes it
    257 pieces, two chunks and the last-arriver join.  The points are 256 distinct ones repeated, so the sum is sum_i (a reps_i) P_i, 256
    terms for the oracle; the equal piece sums also meet in the join (the doubling branch of the complete addition)."""
    a = random.Random(43).randrange(O.N)
    pts = np.ascontiguousarray(base_points[np.arange(n) % 256])
    got = _run(ctxs, scalars_to_array([a] * n), pts, 16)
    reps = np.bincount(np.arange(n) % 256, minlength=256)
    short = scalars_to_array([a * int(r) % O.N for r in reps])
    assert got == _oracle(oracle_lib, short, np.ascontiguousarray(base_points[:256]))


# ---- skewed scalars: empty windows, a size histogram that is mostly zero
@pytest.mark.parametrize("c", (16, 13))
@pytest.mark.parametrize("rest", ("zero", "random"))
def test_skewed_scalars(ctxs, oracle_lib, base_points, c, rest):
    n = 4099
    rnd = random.Random(44)
    sc = [rnd.randrange(1, 1 << 16) if i % 2 else (0 if rest == "zero" else rnd.randrange(O.N)) for i in range(n)]
    sc = scalars_to_array(sc)
    pts = np.ascontiguousarray(base_points[:n])
    assert _run(ctxs, sc, pts, c) == _oracle(oracle_lib, sc, pts)


# ---- special points inside a bucket
@pytest.mark.parametrize("c", WINDOWS)
def test_special_points_inside_a_bucket(ctxs, oracle_lib, base_points, c):
    """Entries of one scalar share a bucket in every window, in input order.  Groups of equal scalars hold (P, -P, Q): the accumulator
    returns to infinity and goes on; (P, P, Q): the doubling branch right after the load; (P, P, -P, -P, P): doubling, back to P (an
    addition whose x differs), to infinity, on; (inf, P), (P, inf, Q), (inf, inf): infinity first, inside, alone.  Zero scalars only shift
    positions."""
    rnd = random.Random(45)
    n = 2003
    sc = [rnd.randrange(O.N) for _ in range(n)]
    pts = base_points[:n].copy()

    def neg(row):
        r = row.copy()
        r[4:] = int_to_limbs((O.P - limbs_to_int(row[4:])) % O.P)
        return r

    i = 10
    for k in range(40):
        kind = k % 6
        P = pts[i].copy()
        if kind == 0:
            grp = [P, neg(P), pts[i + 2]]
        elif kind == 1:
            grp = [P, P, pts[i + 2]]
        elif kind == 2:
            grp = [P, P, neg(P), neg(P), P]
        elif kind == 3:
            grp = [np.zeros(8, dtype=np.uint64), P]
        elif kind == 4:
            grp = [P, np.zeros(8, dtype=np.uint64), pts[i + 2]]
        else:
            grp = [np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)]
        for j, row in enumerate(grp):
            pts[i + j] = row
            sc[i + j] = sc[i]
        i += len(grp) + 3
    for j in range(0, n, 97):
        sc[j] = 0
    sc = scalars_to_array(sc)
    assert _run(ctxs, sc, pts, c) == _oracle(oracle_lib, sc, pts)


# ---- carry window
def _digits16(s):
    """the library's signed 16-bit digits of a scalar (csrc/recode.hip.h), as tests/test_gpu_msm_sort_ranges.py restates them"""
    v = min(s, O.N - s)
    sp = v + sum(1 << (16 * w + 15) for w in range(17))
    return [((sp >> (16 * w)) & 0xFFFF) - (1 << 15) for w in range(17)]


@pytest.mark.parametrize("c", WINDOWS)
def test_carry_window(ctxs, oracle_lib, base_points, c):
    """scalars whose fold min(s, n - s) lies just below 2^255: the top digit wraps and the carry window gets entries"""
    half = (O.N - 1) // 2
    sc = []
    for k in range(40):
        sc += [half - k, half + 1 + k]
    assert any(_digits16(s)[16] for s in sc)
    rnd = random.Random(46)
    sc += [rnd.randrange(O.N) for _ in range(200 - len(sc) + 11)]
    sc = scalars_to_array(sc)
    pts = np.ascontiguousarray(base_points[:sc.shape[0]])
    assert _run(ctxs, sc, pts, c) == _oracle(oracle_lib, sc, pts)


# ---- stale workspace
@pytest.mark.parametrize("c", (16, 13))
def test_stale_workspace(ctxs, oracle_lib, base_points, c):
    """a sized call after a larger one with other inputs on the same contexts, then the larger one again: nothing of the bucket array, the
    items or the piece slots is cleared between calls.  The large call has heavy buckets (a quarter of its scalars are equal)."""
    rnd = random.Random(47)
    n_big, n_small = 20011, 1000
    a = rnd.randrange(O.N)
    big = scalars_to_array([a if i % 4 == 0 else rnd.randrange(O.N) for i in range(n_big)])
    big_pts = np.ascontiguousarray(base_points[np.arange(n_big) % 4099])
    few = [0] * n_small
    for i in (0, 63, 64, 500, n_small - 1):
        few[i] = rnd.randrange(O.N)
    small_sets = [scalars_to_array(few), scalars_to_array([rnd.randrange(O.N) for _ in range(n_small)]), scalars_to_array([a] * n_small)]
    small_pts = np.ascontiguousarray(base_points[5000:5000 + n_small])
    first = _run(ctxs, big, big_pts, c)
    for sc in small_sets:
        assert _run(ctxs, sc, small_pts, c) == _oracle(oracle_lib, sc, small_pts)
        assert _run(ctxs, big, big_pts, c) == first
    assert first is not None


def test_batched_and_registered_basis_calls_keep_the_slices(ctxs, oracle_lib, base_points):
    """the gate: a batch and a registered basis on the sized context run k_acc_points"""
    n, batch = 64, 5
    rnd = random.Random(48)
    sc = [[rnd.randrange(O.N) for _ in range(n)] for _ in range(batch)]
    sarr = np.concatenate([scalars_to_array(s) for s in sc])
    parr = np.ascontiguousarray(base_points[:n])
    want = [_oracle(oracle_lib, scalars_to_array(s), parr) for s in sc]
    g = ctxs[0]
    ds, dp = g.to_device(sarr), g.to_device(parr)
    try:
        assert g.msm_device(ds, dp, n, window_bits=16) == want[0] and _last_sized(g) == 1
        assert g.msm_batch_device(ds, dp, n, batch, shared_points=True, window_bits=16) == want
        assert _last_sized(g) == 0
        basis = g.basis(parr, window_bits=16)
        try:
            assert basis.msm(ds, n, 1) == want[:1]
            assert _last_sized(g) == 0
        finally:
            basis.close()
    finally:
        g.free(ds); g.free(dp)
