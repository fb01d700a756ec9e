"""bppp_test_rp_scan_mul: the fixed-scalar walk of bppp_rp_scan alone (csrc/rpseal.hip.h: one lane per point, ONE scalar for the whole launch,
recoded on the host into the two GLV halves) against the oracle's scalar multiplication AND against the quad walk (bppp_test_rp_excess_mul) with
the same scalar repeated in every row.

The scalars are test_seal_scan_host.WALK_SCALARS — 1, 2, n - 1, n, n + 1, 2^255, 2^256 - 1; halves of all-maximal digits, alternating digits and
long runs of zero digits; lambda, lambda +- 1 and halves that are both negative; 8 seeded random ones — the list that file replays on discrete logs
to show that it reaches every class of addition the walk can reach.  The points are G, -G, k G for small k and infinity; the row counts 1, 63, 64,
65 and 257 (a partial wavefront, a whole one, one lane past it, several workgroups).  The oracle's products are computed once per (scalar, point)."""
import ctypes as C

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import capi
from test_gpu_commit_open import _case, _native
from test_seal_scan_host import POINT_LOGS, WALK_SCALARS

pytestmark = pytest.mark.gpu

N = O.N
COUNTS = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def nat(gpu, oracle_lib):
    h = _native(gpu, _case(oracle_lib, "rec_test")[0])
    yield h
    h.close()


@pytest.fixture(scope="module")
def products(oracle_lib):
    """points[j] = POINT_LOGS[j] G (None: infinity) and want[s][j] = WALK_SCALARS[s] points[j] by the oracle"""
    ec, G = oracle_lib, (O.GX, O.GY)
    points = [None if k == 0 else ec.mul(k, G) for k in POINT_LOGS]
    assert points[1] == ec.neg(G)
    want = [[None if p is None or x % N == 0 else ec.mul(x % N, p) for p in points] for x in WALK_SCALARS]
    return points, want


@pytest.mark.parametrize("count", COUNTS)
def test_lane_walk_equals_oracle_and_quad_walk(gpu, nat, products, count):
    points, want = products
    tl, g = capi.load_test_library(), nat.gpu
    rows = [(3 * i + count) % len(points) for i in range(count)]               # every point at every count but 1; another start per count
    d_pts, d_lane, d_quad = g.to_device(capi.points_to_array([points[j] for j in rows])), g.alloc(64 * count), g.alloc(64 * count)
    try:
        for s, x in enumerate(WALK_SCALARS):
            scalar = capi.int_to_limbs(x)
            d_sc = g.to_device(capi.scalars_to_array([x] * count))
            try:
                g.upload(d_lane, np.full((count, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
                assert tl.bppp_test_rp_scan_mul(nat.h, count, C.c_void_p(scalar.ctypes.data), d_pts, d_lane) == 0
                assert tl.bppp_test_rp_excess_mul(nat.h, count, d_sc, d_pts, d_quad) == 0
                lane, quad = g.download(d_lane, (count, 8), np.uint64), g.download(d_quad, (count, 8), np.uint64)
            finally:
                g.free(d_sc)
            assert [capi.array_to_point(lane[i]) for i in range(count)] == [want[s][j] for j in rows], hex(x)
            assert np.array_equal(lane, quad), hex(x)
    finally:
        for q in (d_pts, d_lane, d_quad):
            g.free(q)


def test_hook_refuses_bad_arguments(gpu, nat):
    tl, g = capi.load_test_library(), nat.gpu
    scalar = capi.int_to_limbs(5)
    d = g.alloc(64)
    try:
        for args in ((0, C.c_void_p(scalar.ctypes.data), d, d), (1, None, d, d), (1, C.c_void_p(scalar.ctypes.data), None, d), (1, C.c_void_p(scalar.ctypes.data), d, None)):
            assert tl.bppp_test_rp_scan_mul(nat.h, *args) == -1
    finally:
        g.free(d)
