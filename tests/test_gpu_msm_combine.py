"""The host's window combine (csrc/hostcurve.hpp window_combine_host) behind every MSM route that ends on the host: the one-launch small route
(window 0; 43 windows at c = 6, one and three slices), balanced 13-bit windows and 16-bit windows with the marginal (W1, W2) sums.  Results are
compared with the oracle's innerProduct (oracle/pyoracle.py) as tests/test_gpu_msm.py does.  The inputs put the combine in its special cases:
upper window sums that are all infinity, a total of infinity, a single addition onto an infinite accumulator, and a scalar whose every window
is in use."""
import ctypes
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd.capi import points_to_array, scalars_to_array

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)
ROUTES = [(0, 64), (0, 3000), (13, 1000), (16, 1000)]         # (window_bits, terms); window 0 is the small route at these sizes
CASES = ["below_2_16", "cancel", "scalar_one", "scalar_minus_one", "random"]
_want = {}


@pytest.fixture(scope="module")
def base_points():
    return points_to_array(O.hash_points(b"host combine", 1024))


def _inputs(base_points, case, n):
    rnd = random.Random(len(case) * 100003 + n)
    pts = np.ascontiguousarray(base_points[(np.arange(n) * 5 + 3) % 1024])
    if case == "below_2_16":                                  # every window above bit 16 sums to infinity
        sc = [rnd.randrange(1 << 16) for _ in range(n)]
    elif case == "cancel":                                    # s and n - s on the same point: the total is infinity, (0, 0)
        pts[1::2] = pts[0::2]
        sc = []
        for _ in range(n // 2):
            s = rnd.randrange(1, O.N)
            sc += [s, O.N - s]
    elif case == "scalar_one":                                # one term
        return scalars_to_array([1]), np.ascontiguousarray(pts[:1])
    elif case == "scalar_minus_one":
        return scalars_to_array([O.N - 1]), np.ascontiguousarray(pts[:1])
    else:
        sc = [rnd.randrange(O.N) for _ in range(n)]
    return scalars_to_array(sc), pts


def _oracle(ec, key, sc, pts):
    if key not in _want:
        _want[key] = ec.inner_product_raw(sc.ctypes.data_as(U64P), pts.ctypes.data_as(U64P), sc.shape[0])
    return _want[key]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("c,n", ROUTES)
def test_combine_routes_match_oracle(gpu, oracle_lib, base_points, c, n, case):
    sc, pts = _inputs(base_points, case, n)
    want = _oracle(oracle_lib, (case, sc.shape[0] if sc.shape[0] == 1 else n), sc, pts)
    ds, dp = gpu.to_device(sc), gpu.to_device(pts)
    try:
        got = gpu.msm_device(ds, dp, sc.shape[0], window_bits=c)
    finally:
        gpu.free(ds); gpu.free(dp)
    assert got == want
    if case == "cancel":
        assert got is None                                    # (0, 0), infinity
