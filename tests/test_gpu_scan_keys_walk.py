"""bppp_test_rp_scan_keys_mul: the table, the multi-key walk and the batched affine conversion of bppp_rp_scan_keys alone
(csrc/rpscan_keys.hip.h: one lane per point, a LIST of scalars walked one after another inside one launch per tile of keys, one inversion per
point and tile) against the oracle's scalar multiplication AND, per key, byte for byte against the one-key walk (bppp_test_rp_scan_mul) with
that scalar.

The scalars are test_seal_scan_host.WALK_SCALARS, taken cyclically from another start per key count so that n (an accumulator at infinity inside
a point's inversion batch) lands at different places of a tile; tests/test_scan_keys_host.py replays the same list on discrete logs.  The points
are G, -G, k G for small k and infinity (a whole batch at infinity); the row counts 1, 63, 64, 65 and 257; the key counts 1, 2, KT - 1, KT,
KT + 1 and 2 KT + 1 with KT read from the geometry hook.  The oracle's products are computed once per (scalar, point), and the one-key walk's
once per (scalar, row count)."""
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
    want = [[None if p is None or x % N == 0 else ec.mul(x % N, p) for p in points] for x in WALK_SCALARS]
    return points, want


def _geometry(nat, rows, nkeys):
    out = np.zeros(3, dtype=np.uint64)
    assert capi.load_test_library().bppp_test_rp_scan_keys_geometry(nat.h, rows, nkeys, C.c_void_p(out.ctypes.data)) == 0
    return [int(v) for v in out]


@pytest.mark.parametrize("count", COUNTS)
def test_keys_walk_equals_oracle_and_one_key_walk(gpu, nat, products, count):
    points, want = products
    tl, g = capi.load_test_library(), nat.gpu
    KT = _geometry(nat, count, 2**20)[1]
    assert KT >= 3 and _geometry(nat, count, 2)[1] == 2
    key_counts = (1, 2, KT - 1, KT, KT + 1, 2 * KT + 1)
    rows = [(3 * i + count) % len(points) for i in range(count)]               # every point at every count but 1; another start per count
    d_pts, d_one = g.to_device(capi.points_to_array([points[j] for j in rows])), g.alloc(64 * count)
    try:
        one = []                                                               # the one-key walk, once per scalar
        for x in WALK_SCALARS:
            scalar = capi.int_to_limbs(x)
            assert tl.bppp_test_rp_scan_mul(nat.h, count, C.c_void_p(scalar.ctypes.data), d_pts, d_one) == 0
            one.append(g.download(d_one, (count, 8), np.uint64))
        for nk in key_counts:
            picks = [(nk + 7 * k) % len(WALK_SCALARS) for k in range(nk)]      # 7 is coprime to the list's 25: 2 KT + 1 keys walk every scalar
            sc = capi.scalars_to_array([WALK_SCALARS[s] for s in picks])
            d_out = g.to_device(np.full((nk * count, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
            try:
                assert tl.bppp_test_rp_scan_keys_mul(nat.h, nk, C.c_void_p(sc.ctypes.data), count, d_pts, d_out) == 0
                got = g.download(d_out, (nk, count, 8), np.uint64)
            finally:
                g.free(d_out)
            for k, s in enumerate(picks):
                assert np.array_equal(got[k], one[s]), (nk, k, hex(WALK_SCALARS[s]))
                assert [capi.array_to_point(got[k][i]) for i in range(count)] == [want[s][j] for j in rows], (nk, k, hex(WALK_SCALARS[s]))
    finally:
        for q in (d_pts, d_one):
            g.free(q)


def test_hook_refuses_bad_arguments(gpu, nat):
    tl, g = capi.load_test_library(), nat.gpu
    sc = capi.scalars_to_array([5, 7])
    p, d = C.c_void_p(sc.ctypes.data), g.alloc(128)
    try:
        for args in ((0, p, 1, d, d), (2, None, 1, d, d), (2, p, 0, d, d), (2, p, 1, None, d), (2, p, 1, d, None), (2**20 + 1, p, 1, d, d)):
            assert tl.bppp_test_rp_scan_keys_mul(nat.h, *args) == -1
    finally:
        g.free(d)
