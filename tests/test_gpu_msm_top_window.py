"""The MSM's top window without a carry window (csrc/msm.hip window_layout, csrc/recode.hip.h): where the top window has one bit to spare
its digit is stored negated and its entries' signs flipped, instead of a further window that only catches the carry of d = 2^(cw-1).
Results are compared with the oracle's innerProduct (oracle/pyoracle.py) as tests/test_gpu_msm.py does; the plan's window count is read
through bppp_test_last_windows.  The scalars sit on the boundaries of that top digit: (n - 1) / 2, the largest folded value, has the top
field 0x7FFF and the window below 0xFFFF at 16 bits, so with the carry it is d = 2^15 exactly."""
import ctypes
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd.capi import points_to_array, scalars_to_array

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)
HALF = (O.N - 1) // 2
EDGE = [HALF, HALF + 1, O.N - 1, 1, 0, (2**255 - 1) % O.N, HALF - 1, HALF + 2, 2**255 % O.N]
EDGE += [(k << 240) % O.N for k in (1, 2, 0x3FFF, 0x4000, 0x7FFF, 0x8000, 0xFFFF)]
EDGE += [((k << 240) + e) % O.N for k in (1, 2, 0x3FFF, 0x4000, 0x7FFF, 0x8000, 0xFFFF) for e in (1, -1)]


def _windows(c, balanced):
    """window_layout of csrc/msm.hip: balanced widths for one MSM whose c does not divide 256, else uniform"""
    if balanced and c >= 3 and 256 % c:
        return -(-256 // c)
    return -(-255 // c) + (1 if 255 % c == 0 else 0)


def _last_windows(g):
    from bulletproofspp_amd.capi import load_test_library
    v = ctypes.c_int(-2)
    assert load_test_library().bppp_test_last_windows(g.h, ctypes.byref(v)) == 0
    return v.value


def _oracle(ec, sc, pts):
    sc, pts = np.ascontiguousarray(sc), np.ascontiguousarray(pts)
    return ec.inner_product_raw(sc.ctypes.data_as(U64P), pts.ctypes.data_as(U64P), sc.shape[0])


@pytest.fixture(scope="module")
def base_points():
    return points_to_array(O.hash_points(b"top window", 2048))


def _case(base_points, n, seed):
    """the edge scalars with either sign of every one of them present, a random remainder, a zero point; points repeat from 2048 hashed ones"""
    rnd = random.Random(seed)
    sc = EDGE + [rnd.randrange(O.N) for _ in range(n - len(EDGE))]
    rnd.shuffle(sc)
    pts = np.ascontiguousarray(base_points[(np.arange(n) * 7 + seed) % 2048])
    pts[n // 3] = 0                                          # affine (0, 0): infinity
    return scalars_to_array(sc), pts


def _msm(g, sc, pts, c):
    ds, dp = g.to_device(sc), g.to_device(pts)
    try:
        return g.msm_device(ds, dp, sc.shape[0], window_bits=c)
    finally:
        g.free(ds); g.free(dp)


def test_the_edge_scalars_hit_the_top_digit_boundary():
    """what the other tests rely on, from the format alone: at c = 16 the top field of (n - 1) / 2 is 0x7FFF, the window below it 0xFFFF,
    and the unbiased top digit of v + K is 2^15 — the one value the biased field had no room for"""
    assert HALF >> 240 == 0x7FFF and (HALF >> 224) & 0xFFFF == 0xFFFF and HALF < 2**255
    k = sum(1 << (16 * w + 15) for w in range(15))
    assert (HALF + k) >> 240 == 1 << 15
    assert min(HALF + 1, O.N - (HALF + 1)) == HALF        # (n + 1) / 2 folds to the same value, point negated


@pytest.mark.parametrize("c", list(range(2, 17)))
def test_edge_scalars_every_width(gpu, oracle_lib, base_points, c):
    sc, pts = _case(base_points, 300, c)
    assert _msm(gpu, sc, pts, c) == _oracle(oracle_lib, sc, pts)
    assert _last_windows(gpu) == _windows(c, True)


@pytest.mark.parametrize("n", [300, 5000])
def test_edge_scalars_small_route(gpu, oracle_lib, base_points, n):
    sc, pts = _case(base_points, n, n)
    assert gpu.msm(sc, pts) == _oracle(oracle_lib, sc, pts)
    assert _last_windows(gpu) == 43                          # k_msm_small, c = 6: 41 windows of 6 bits and 2 of 5


@pytest.mark.parametrize("n,c", [(4096, 11), (22016, 12), (43782, 13)])
def test_edge_scalars_mid_sizes(oracle_lib, base_points, n, c, monkeypatch):
    """the sizes at which choose_window takes c = 11, 12 and 13 (the small route is switched off for the first)"""
    import bulletproofspp_amd as b
    monkeypatch.setenv("BPPP_MSM_NO_SMALL", "1")
    g = b.Bppp(0)
    try:
        sc, pts = _case(base_points, n, n)
        assert g.msm(sc, pts) == _oracle(oracle_lib, sc, pts)
        assert _last_windows(g) == -(-256 // c)
    finally:
        g.close()


@pytest.mark.parametrize("s", [HALF, HALF + 1])
def test_all_terms_in_the_extreme_bucket(gpu, oracle_lib, base_points, s):
    """2048 distinct points, every scalar (n - 1) / 2 or (n + 1) / 2: the top window's entries all lie in its last bucket, |digit| = 2^(cw-1),
    on the small route, with balanced narrow windows (c = 13) and with 16-bit windows"""
    n = 2048
    sc, pts = scalars_to_array([s] * n), base_points
    want = _oracle(oracle_lib, sc, pts)
    assert want is not None
    assert gpu.msm(sc, pts) == want
    for c in (13, 16):
        assert _msm(gpu, sc, pts, c) == want


def test_window_count(gpu, base_points):
    sc, pts = _case(base_points, 300, 99)
    n = sc.shape[0]
    for c, w in ((16, 16), (13, 20), (8, 32)):
        _msm(gpu, sc, pts, c)
        assert _last_windows(gpu) == w, c
    ds, dp = gpu.to_device(np.concatenate([sc] * 5)), gpu.to_device(pts)
    try:
        # uniform widths (a batch): 15 divides 255, the top window is full and its carry window stays
        gpu.msm_batch_device(ds, dp, n, 5, shared_points=True, window_bits=15)
        assert _last_windows(gpu) == 256 // 15 + 1 == 18
        gpu.msm_batch_device(ds, dp, n, 5, shared_points=True, window_bits=16)
        assert _last_windows(gpu) == 16
        # a registered basis keeps its 256 / c + 1 table rows
        for c in (16, 8):
            basis = gpu.basis(pts, window_bits=c)
            try:
                basis.msm(ds, n, 1)
                assert _last_windows(gpu) == 256 // c + 1, c
            finally:
                basis.close()
    finally:
        gpu.free(ds); gpu.free(dp)


@pytest.mark.parametrize("batch,c", [(8, 0), (8, 8), (8, 15), (8, 16), (3, 8)])
def test_batch_route(gpu, oracle_lib, base_points, batch, c):
    """instances of 200 terms with the edge scalars at different places; 8 go through k_window_combine, 3 through the host's combine"""
    n = 200
    cases = [_case(base_points, n, 500 + b) for b in range(batch)]
    pts = cases[0][1]
    ds, dp = gpu.to_device(np.concatenate([s for s, _ in cases])), gpu.to_device(pts)
    try:
        got = gpu.msm_batch_device(ds, dp, n, batch, shared_points=True, window_bits=c)
    finally:
        gpu.free(ds); gpu.free(dp)
    assert got == [_oracle(oracle_lib, s, pts) for s, _ in cases]
    if c:
        assert _last_windows(gpu) == _windows(c, False)
