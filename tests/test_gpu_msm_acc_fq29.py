"""Whole MSMs on the sized route with the accumulator in 9 x 29-bit limbs (k_acc_points_sized29; BPPP_ACC_FQ29, read when a context is created,
beside BPPP_ACC_SIZED).  A context with BPPP_ACC_SIZED=1 BPPP_ACC_FQ29=1 runs beside one with BPPP_ACC_FQ29=0 (k_acc_points_sized on 10 x 26);
both report their kernel through bppp_test_last_acc_fq29, and every result is compared with the other context's and with the oracle's.
Explicit window widths 5, 13 and 16 keep a small input off the one-launch route."""
import ctypes
import os
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd.capi import int_to_limbs, limbs_to_int, load_test_library, points_to_array, scalars_to_array

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)
CAP = 128                         # ACC_CAP of csrc/msm.hip
WINDOWS = (5, 13, 16)


def _oracle(ec, sc, pts):
    sc, pts = np.ascontiguousarray(sc), np.ascontiguousarray(pts)
    return ec.inner_product_raw(sc.ctypes.data_as(U64P), pts.ctypes.data_as(U64P), sc.shape[0])


@pytest.fixture(scope="module")
def ctxs():
    """[fq29, fq26], both sized: the environment is read at creation and restored afterwards"""
    import bulletproofspp_amd as b
    old = {k: os.environ.get(k) for k in ("BPPP_ACC_SIZED", "BPPP_ACC_FQ29")}
    out = []
    try:
        os.environ["BPPP_ACC_SIZED"] = "1"
        for v in ("1", "0"):
            os.environ["BPPP_ACC_FQ29"] = v
            out.append(b.Bppp(0))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield out
    for g in out:
        g.close()


@pytest.fixture(scope="module")
def base_points():
    return points_to_array(O.hash_points(b"acc fq29", 3000))


def _last(g, name):
    v = ctypes.c_int(-2)
    assert getattr(load_test_library(), name)(g.h, ctypes.byref(v)) == 0
    return v.value


def _run(ctxs, sc_arr, pt_arr, c):
    n = sc_arr.shape[0]
    out = []
    for want, g in zip((1, 0), ctxs):
        ds, dp = g.to_device(sc_arr), g.to_device(pt_arr)
        try:
            out.append(g.msm_device(ds, dp, n, window_bits=c))
        finally:
            g.free(ds); g.free(dp)
        assert _last(g, "bppp_test_last_acc_sized") == 1
        assert _last(g, "bppp_test_last_acc_fq29") == want
    assert out[0] == out[1], ("fq29 != fq26", c, n)
    return out[0]


def _neg(row):
    r = row.copy()
    r[4:] = int_to_limbs((O.P - limbs_to_int(row[4:])) % O.P)
    return r


@pytest.mark.parametrize("n", (300, 3000))
@pytest.mark.parametrize("c", WINDOWS)
def test_random_terms(ctxs, oracle_lib, base_points, c, n):
    rnd = random.Random(100 * c + n)
    sc = scalars_to_array([rnd.randrange(O.N) for _ in range(n)])
    pts = np.ascontiguousarray(base_points[:n])
    assert _run(ctxs, sc, pts, c) == _oracle(oracle_lib, sc, pts)


@pytest.mark.parametrize("c", WINDOWS)
def test_one_bucket_of_several_pieces(ctxs, oracle_lib, base_points, c):
    """all scalars equal, n = 2 CAP + 44: in every window one bucket of three pieces (two full, one short), joined by k_merge_heavy<true>"""
    n = 2 * CAP + 44
    sc = scalars_to_array([random.Random(c).randrange(O.N)] * n)
    pts = np.ascontiguousarray(base_points[:n])
    assert _run(ctxs, sc, pts, c) == _oracle(oracle_lib, sc, pts)


@pytest.mark.parametrize("c", WINDOWS)
def test_repeated_and_opposite_points_under_equal_scalars(ctxs, oracle_lib, base_points, c):
    """one bucket per window whose entries are P, P, -P, Q, Q, Q, -Q, ...: doublings, returns to infinity, and equal piece sums in the join"""
    n = CAP + 72
    pts = base_points[:n].copy()
    for i in range(0, n - 8, 8):
        pts[i + 1] = pts[i]; pts[i + 2] = _neg(pts[i]); pts[i + 4] = pts[i + 3]; pts[i + 5] = pts[i + 3]; pts[i + 6] = _neg(pts[i + 3])
    pts[CAP:CAP + 40] = pts[:40]                                  # the second piece starts like the first
    sc = scalars_to_array([random.Random(7 + c).randrange(O.N)] * n)
    assert _run(ctxs, sc, pts, c) == _oracle(oracle_lib, sc, pts)


@pytest.mark.parametrize("c", WINDOWS)
def test_infinity_points_and_zero_scalars(ctxs, oracle_lib, base_points, c):
    rnd = random.Random(11 + c)
    n = 301
    sc = [rnd.randrange(O.N) for _ in range(n)]
    pts = base_points[:n].copy()
    for i in range(0, n, 7):
        pts[i] = 0                                                # infinity
    for i in range(3, n, 11):
        sc[i] = 0
    for i in range(20, 60):                                       # a shared bucket with infinity first, inside and last
        sc[i] = sc[20]
    pts[20] = 0; pts[33] = 0; pts[59] = 0
    sc = scalars_to_array(sc)
    assert _run(ctxs, sc, pts, c) == _oracle(oracle_lib, sc, pts)


@pytest.mark.parametrize("c", (13, 16))
def test_two_calls_on_one_context(ctxs, oracle_lib, base_points, c):
    """a larger call with a heavy bucket, a smaller one with other inputs, the larger one again: nothing of the bucket array, the items or the
    piece slots is cleared between calls"""
    rnd = random.Random(13 + c)
    a = rnd.randrange(O.N)
    big = scalars_to_array([a if i % 4 == 0 else rnd.randrange(O.N) for i in range(3000)])
    big_pts = np.ascontiguousarray(base_points[:3000])
    small = scalars_to_array([rnd.randrange(O.N) for _ in range(300)])
    small_pts = np.ascontiguousarray(base_points[1000:1300])
    first = _run(ctxs, big, big_pts, c)
    assert first == _oracle(oracle_lib, big, big_pts)
    assert _run(ctxs, small, small_pts, c) == _oracle(oracle_lib, small, small_pts)
    assert _run(ctxs, big, big_pts, c) == first
