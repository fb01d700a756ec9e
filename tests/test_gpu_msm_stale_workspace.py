"""The general MSM pipeline no longer clears its bucket array between calls: an empty bucket is marked by k_merge, every other one is
written before a reduction reads it.  These tests run a SPARSE call right after a DENSE one on the same context (same n, same window
width, hence the same workspace layout), so that a bucket left over from the first call would show in the second; and they run
k_acc_points (13-bit windows, batches) and the sized accumulation (16-bit windows) on inputs that reach every branch of the kernel.
Every expected value comes from the oracle (oracle/pyoracle.py), never from the library."""
import ctypes
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd.capi import int_to_limbs, limbs_to_int, points_to_array, scalars_to_array

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)
N_BIG = (1 << 14) + 37          # above the one-launch route (> 8192 terms), not a multiple of 64


def _oracle(ec, sc, pts):
    sc, pts = np.ascontiguousarray(sc), np.ascontiguousarray(pts)
    return ec.inner_product_raw(sc.ctypes.data_as(U64P), pts.ctypes.data_as(U64P), sc.shape[0])


@pytest.fixture(scope="module")
def big_points():
    return points_to_array(O.hash_points(b"stale workspace", N_BIG))


def _scalar_sets(n):
    rnd = random.Random(20)
    dense = [rnd.randrange(O.N) for _ in range(n)]
    few = [0] * n
    for i in (0, 63, 64, 4095, 4096, n - 1):
        few[i] = rnd.randrange(O.N)
    return {
        "dense": dense,
        "all_equal": [dense[0]] * n,                                   # one bucket per window holds every entry (heavy merge)
        "few_nonzero": few,                                            # nearly every bucket empty
        "one_window": [rnd.randrange(1, 1 << 12) for _ in range(n)],   # digits confined to the lowest window
    }


@pytest.fixture(scope="module")
def big_cases(big_points, oracle_lib):
    sets = _scalar_sets(N_BIG)
    return {k: (scalars_to_array(v), _oracle(oracle_lib, scalars_to_array(v), big_points)) for k, v in sets.items()}


@pytest.mark.parametrize("c", [13, 16])
def test_sparse_call_after_dense_call(gpu, big_points, big_cases, c):
    dp = gpu.to_device(big_points)
    try:
        for name in ("dense", "all_equal", "dense", "few_nonzero", "dense", "one_window"):
            sc, want = big_cases[name]
            ds = gpu.to_device(sc)
            try:
                assert gpu.msm_device(ds, dp, N_BIG, window_bits=c) == want, (c, name)
            finally:
                gpu.free(ds)
    finally:
        gpu.free(dp)


def test_sparse_batch_after_dense_batch_grouped_reduction(gpu, oracle_lib):
    """batch > 4 with thousands of small windows: the k_reduce_groups route (batch * windows >= 4096, <= 256 buckets each)"""
    n, batch, c = 40, 80, 5
    rnd = random.Random(21)
    pts = O.hash_points(b"stale batch", n)
    dense = [[rnd.randrange(O.N) for _ in range(n)] for _ in range(batch)]
    sparse = [[0] * n for _ in range(batch)]
    for b in range(0, batch, 3):
        sparse[b][b % n] = rnd.randrange(O.N)
    sparse[7] = [3] * n
    dp = gpu.to_device(points_to_array(pts))
    try:
        for sc in (dense, sparse, dense, sparse):
            ds = gpu.to_device(np.concatenate([scalars_to_array(s) for s in sc]))
            try:
                got = gpu.msm_batch_device(ds, dp, n, batch, shared_points=True, window_bits=c)
            finally:
                gpu.free(ds)
            for b in range(batch):
                assert got[b] == oracle_lib.inner_product(list(zip(sc[b], pts))), b
    finally:
        gpu.free(dp)


@pytest.mark.parametrize("batch", [1, 6])
def test_sparse_call_after_dense_call_registered_basis(gpu, oracle_lib, batch):
    """table_stride != 0: the windows of an instance share one bucket set"""
    n, c = 9000, 13
    rnd = random.Random(22)
    pts = O.hash_points(b"stale basis", 64)
    pts = [pts[i % 64] for i in range(n)]
    parr = points_to_array(pts)
    basis = gpu.basis(parr, window_bits=c, batch_hint=batch)
    try:
        dense = [[rnd.randrange(O.N) for _ in range(n)] for _ in range(batch)]
        sparse = [[0] * n for _ in range(batch)]
        for b in range(batch):
            for i in (b, 64 + b, n - 1 - b):
                sparse[b][i] = rnd.randrange(O.N)
        for sc in (dense, sparse):
            arrs = [scalars_to_array(s) for s in sc]
            ds = gpu.to_device(np.concatenate(arrs))
            try:
                got = basis.msm(ds, n, batch)
            finally:
                gpu.free(ds)
            for b in range(batch):
                assert got[b] == _oracle(oracle_lib, arrs[b], parr), b
    finally:
        basis.close()


# ---- the accumulate kernels on constructed inputs
def _run(g, sc_arr, pt_arr, n, c):
    ds, dp = g.to_device(sc_arr), g.to_device(pt_arr)
    try:
        return g.msm_device(ds, dp, n, window_bits=c)
    finally:
        g.free(ds); g.free(dp)


@pytest.mark.parametrize("c", [13, 16])
def test_acc_kernel_edge_inputs(gpu, oracle_lib, big_points, c):
    """Infinity points, zero scalars, repeated and cancelling points inside a run, n not a multiple of 64.  One input in 64 is the point at
    infinity: slices are cut in SORTED order (a lane owns L consecutive sorted entries), so with ~5000 slices per call and a 1-in-64 density
    such entries fall on first and last slice positions by chance many times over, they are not placed there.  Zero scalars never reach
    the kernel (the sort drops zero digits); they shift every later entry's position.  The constructed boundary case is
    test_acc_kernel_runs_that_end_on_slice_boundaries."""
    n = N_BIG
    rnd = random.Random(23)
    sc = [rnd.randrange(O.N) for _ in range(n)]
    pts = big_points.copy()
    for i in range(0, n, 64):
        sc[i] = 0
        pts[(i + 63) % n] = 0                      # affine (0, 0): infinity
    for i in range(100, 4000, 7):                  # P, P, -P with one scalar: the same bucket in every window, a doubling and a cancellation in the run
        pts[i + 1] = pts[i]
        pts[i + 2] = pts[i]
        pts[i + 2, 4:] = int_to_limbs((O.P - limbs_to_int(pts[i, 4:])) % O.P)
        sc[i + 1] = sc[i + 2] = sc[i]
    sarr = scalars_to_array(sc)
    assert _run(gpu, sarr, pts, n, c) == _oracle(oracle_lib, sarr, pts)


@pytest.mark.parametrize("c", [13, 16])
def test_acc_kernel_runs_that_end_on_slice_boundaries(gpu, oracle_lib, big_points, c):
    """Scalars below 2^12 put every entry in window 0, bucket = the scalar: the sorted order is by scalar, then by input index.  Bucket m
    (m = 1, 2, ...) gets exactly 8 * m entries, so with L = 8 entries per lane at this size every run starts AND ends on a slice boundary
    (a multiple of every power of two <= 8), and infinity points sit first and last in their runs.  Whatever L the plan picks, run lengths
    8, 16, 24, ... put boundaries of runs on boundaries of slices."""
    sc, pts = [], []
    m, k = 1, 0
    src = big_points
    while len(sc) + 8 * m <= 4096 + 8192:
        for j in range(8 * m):
            sc.append(m)
            pts.append(src[k % N_BIG]); k += 1
        pts[-8 * m] = np.zeros(8, dtype=np.uint64)           # first of its run: infinity
        if m % 2:
            pts[-1] = np.zeros(8, dtype=np.uint64)           # last of its run: infinity
        m += 1
    n = len(sc)
    assert n > 8192
    sarr, parr = scalars_to_array(sc), np.ascontiguousarray(np.stack(pts))
    assert _run(gpu, sarr, parr, n, c) == _oracle(oracle_lib, sarr, parr)


@pytest.mark.parametrize("c", [13, 16])
def test_acc_kernel_one_bucket_holds_every_entry(gpu, big_points, big_cases, c):
    sc, want = big_cases["all_equal"]
    assert _run(gpu, sc, big_points, N_BIG, c) == want


@pytest.mark.parametrize("shared", [0, 1, 2])
def test_acc_kernel_shared_points_modes(gpu, oracle_lib, shared):
    """shared_pts = 0 (a basis per instance), 1 (one basis), d = 2 (one basis per two consecutive instances)"""
    n, batch = 333, 6
    rnd = random.Random(24 + shared)
    nb = {0: batch, 1: 1, 2: batch // 2}[shared]
    base = O.hash_points(b"stale shared", n * nb)
    bases = [base[k * n:(k + 1) * n] for k in range(nb)]
    of = {0: lambda b: b, 1: lambda b: 0, 2: lambda b: b // 2}[shared]
    sc = [[rnd.randrange(O.N) if rnd.random() > 0.2 else 0 for _ in range(n)] for _ in range(batch)]
    sarr = np.concatenate([scalars_to_array(s) for s in sc])
    parr = np.concatenate([points_to_array(p) for p in bases])
    ds, dp = gpu.to_device(sarr), gpu.to_device(parr)
    try:
        got = gpu.msm_batch_device(ds, dp, n, batch, shared_points=shared)
    finally:
        gpu.free(ds); gpu.free(dp)
    assert got == [oracle_lib.inner_product(list(zip(sc[b], bases[of(b)]))) for b in range(batch)]
