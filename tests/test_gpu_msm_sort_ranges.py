"""The ranged scatter of the MSM's counting sort (k_scatter_ranges; BPPP_SORT_RANGES = Q bucket ranges per window, read when a context is
created): one MSM over arbitrary points with 16-bit windows places its sorted entries from (window, range, chunk) workgroups.  Contexts
with Q = 2 and Q = 4, each with the plan's chunk count and with a forced odd one (BPPP_HIST_CH=5), must give bit for bit what the Q = 0
context (k_scatter) gives; where said, that value is also the oracle's (oracle/pyoracle.py).  window_bits = 16 is passed so that small
inputs take the general pipeline with 2^15 buckets per window."""
import ctypes
import os
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd.capi import points_to_array, scalars_to_array

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)
C, M, W = 16, 1 << 15, 17
N_ODD = 20011                     # not a multiple of 8: the chunk ends fall inside a 16-byte group of digits
CONFIGS = [(0, None), (2, None), (4, None), (2, "5"), (4, "5")]     # (BPPP_SORT_RANGES, BPPP_HIST_CH); the first is the comparison


def _oracle(ec, sc, pts):
    sc, pts = np.ascontiguousarray(sc), np.ascontiguousarray(pts)
    return ec.inner_product_raw(sc.ctypes.data_as(U64P), pts.ctypes.data_as(U64P), sc.shape[0])


@pytest.fixture(scope="module")
def ctxs():
    """one context per entry of CONFIGS; the environment is read at creation and restored afterwards"""
    import bulletproofspp_amd as b
    old = {k: os.environ.get(k) for k in ("BPPP_SORT_RANGES", "BPPP_HIST_CH")}
    out = []
    try:
        for q, ch in CONFIGS:
            os.environ["BPPP_SORT_RANGES"] = str(q)
            if ch is None:
                os.environ.pop("BPPP_HIST_CH", None)
            else:
                os.environ["BPPP_HIST_CH"] = ch
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
    return points_to_array(O.hash_points(b"sort ranges", 256))


def _points(base_points, n):
    """n points from 256 hashed ones (they repeat across buckets, as in test_msm_2_16_matches_oracle)"""
    return np.ascontiguousarray(base_points[np.arange(n) % 256])


def _last_q(g):
    from bulletproofspp_amd.capi import load_test_library
    q = ctypes.c_int(-2)
    assert load_test_library().bppp_test_last_sort_ranges(g.h, ctypes.byref(q)) == 0
    return q.value


def _run_all(ctxs, sc_arr, pt_arr):
    """the MSM on every context, window_bits = 16; each context reports the scatter it was created for"""
    n = sc_arr.shape[0]
    out = []
    for (q, _), g in zip(CONFIGS, ctxs):
        ds, dp = g.to_device(sc_arr), g.to_device(pt_arr)
        try:
            out.append(g.msm_device(ds, dp, n, window_bits=C))
        finally:
            g.free(ds); g.free(dp)
        assert _last_q(g) == q, (q, _last_q(g))
    return out


def _all_equal(got, want=None):
    for (q, ch), r in zip(CONFIGS, got):
        assert r == got[0], ("Q", q, "CH", ch)
    if want is not None:
        assert got[0] == want


def _digits(s):
    """the library's signed 16-bit digits of a scalar (csrc/recode.hip.h): s > n - s is folded, then digit = field - 2^15 of v + K"""
    v = min(s, O.N - s)
    sp = v + sum(1 << (C * w + C - 1) for w in range(W))
    return [((sp >> (C * w)) & 0xFFFF) - M for w in range(W)]


def test_random_scalars_odd_length(ctxs, oracle_lib, base_points):
    rnd = random.Random(31)
    sc = scalars_to_array([rnd.randrange(O.N) for _ in range(N_ODD)])
    pts = _points(base_points, N_ODD)
    _all_equal(_run_all(ctxs, sc, pts), _oracle(oracle_lib, sc, pts))


def test_digits_on_the_range_borders(ctxs, oracle_lib, base_points):
    """|digit| = k M / Q - 1, k M / Q, k M / Q + 1 for every k of Q = 2 and Q = 4, and 1 and M, in the low, a middle and the top window, with
    either sign; and the sign-boundary scalars of test_msm_every_window_width, which carry into the extra top window"""
    mags = {1, M}
    for q in (2, 4):
        for k in range(1, q + 1):
            mags |= {k * M // q - 1, k * M // q, k * M // q + 1}
    sc = []
    for w in (0, 7, 15):
        for m in sorted(mags):
            s = (m << (C * w)) % O.N
            sc += [s, O.N - s]
    sc += [(O.N - 1) // 2, (O.N + 1) // 2, (O.N - 1) // 2 - 1, (O.N + 1) // 2 + 1, O.N - 1, 1, 2**255 % O.N, 2**254, 2**254 - 1]
    # what the scatter sees: every border magnitude up to M in each of the three windows, and a non-empty carry window
    digs = [_digits(s) for s in sc]
    for w in (0, 7, 15):
        seen = {abs(d[w]) for d in digs}
        assert {m for m in mags if m <= M} <= seen, (w, sorted(m for m in mags if m <= M and m not in seen))
    assert any(d[W - 1] for d in digs)
    rnd = random.Random(32)
    sc += [rnd.randrange(O.N) for _ in range(301 - len(sc) % 8)]          # odd length again
    sc = scalars_to_array(sc)
    pts = _points(base_points, sc.shape[0])
    _all_equal(_run_all(ctxs, sc, pts), _oracle(oracle_lib, sc, pts))


def test_skewed_scalars(ctxs, base_points):
    """all scalars equal: one bucket per window holds every entry (one range gets everything, the heavy merge runs); then two values
    whose digits lie in different ranges of every window"""
    pts = _points(base_points, N_ODD)
    a = sum(0x0123 << (C * w) for w in range(15))           # |digit| 0x0123 in windows 0..14: the first range of Q = 2 and of Q = 4
    b = sum(0x7345 << (C * w) for w in range(15))           # |digit| 0x7345: the last range of both
    assert all(abs(d) == 0x0123 for d in _digits(a)[:15]) and all(abs(d) == 0x7345 for d in _digits(b)[:15])
    _all_equal(_run_all(ctxs, scalars_to_array([a] * N_ODD), pts))
    _all_equal(_run_all(ctxs, scalars_to_array([a if i % 3 else b for i in range(N_ODD)]), pts))


def test_zero_scalars_and_infinity_points(ctxs, oracle_lib, base_points):
    n = 4099
    rnd = random.Random(33)
    sc = [rnd.randrange(O.N) for _ in range(n)]
    pts = _points(base_points, n).copy()
    for i in (0, 7, 8, n - 1):
        sc[i] = 0
    for i in (1, 7, 9, n - 1):
        pts[i] = 0                                          # affine (0, 0): infinity
    sc = scalars_to_array(sc)
    _all_equal(_run_all(ctxs, sc, pts), _oracle(oracle_lib, sc, pts))


def test_stale_workspace(ctxs, base_points):
    """a long call, a short one and the long one again on the same contexts: the third result equals the first"""
    rnd = np.random.default_rng(34)
    cases = []
    for n in (70001, 9001):
        sc = rnd.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rnd.integers(0, 2, size=(n, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64(0x7FFFFFFFFFFFFFFF)           # < 2^255 < n
        cases.append((sc, _points(base_points, n)))
    first = _run_all(ctxs, *cases[0])
    second = _run_all(ctxs, *cases[1])
    third = _run_all(ctxs, *cases[0])
    _all_equal(first)
    _all_equal(second)
    assert third == first and first[0] is not None and second[0] != first[0]


def test_batched_and_registered_basis_calls_keep_the_old_scatter(ctxs, oracle_lib, base_points):
    """the gate: a batch and a registered basis on a ranged context run k_scatter, also with 16-bit windows"""
    n, batch = 64, 5
    rnd = random.Random(35)
    sc = [[rnd.randrange(O.N) for _ in range(n)] for _ in range(batch)]
    sarr = np.concatenate([scalars_to_array(s) for s in sc])
    parr = _points(base_points, n)
    want = [_oracle(oracle_lib, scalars_to_array(s), parr) for s in sc]
    for (q, ch), g in zip(CONFIGS, ctxs):
        if ch is not None:
            continue
        ds, dp = g.to_device(sarr), g.to_device(parr)
        try:
            assert g.msm_device(ds, dp, n, window_bits=C) == want[0] and _last_q(g) == q
            assert g.msm_batch_device(ds, dp, n, batch, shared_points=True, window_bits=C) == want
            assert _last_q(g) == 0, q
            assert g.msm_device(ds, dp, n, window_bits=C) == want[0] and _last_q(g) == q
            basis = g.basis(parr, window_bits=C)
            try:
                assert basis.msm(ds, n, 1) == want[:1]
                assert _last_q(g) == 0, q
            finally:
                basis.close()
        finally:
            g.free(ds); g.free(dp)
