"""The chain forms of the XYZZ point operations (csrc/ec.hip.h: xyzz_add_chain, xyzz_dbl_chain — the products of one addition issued in
pairs, csrc/fq26.hip.h) against xyzz_add / xyzz_dbl, raw limbs bit for bit, and against the oracle's group law; then the MSM kernels that
use them (k_reduce_marg with its prefetching serial loop, both tails of the bucket reduction, k_merge_heavy) against the oracle's
innerProduct (oracle/pyoracle.py), as tests/test_gpu_msm.py does, at the smallest shapes that reach each of them."""
import ctypes
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd.capi import array_to_point, load_test_library, points_to_array, scalars_to_array

pytestmark = pytest.mark.gpu


# ---- group law
def _chain_op(gpu, op, ps, qs):
    A, B = points_to_array(ps), points_to_array(qs)
    out = np.zeros_like(A)
    raw = np.zeros((len(ps), 80), dtype=np.uint32)
    rc = load_test_library().bppp_test_point_chain(gpu.h, op, A.ctypes.data, B.ctypes.data, len(ps), out.ctypes.data, raw.ctypes.data)
    assert rc == 0, gpu.lib.bppp_last_error(gpu.h)
    return [array_to_point(out[i]) for i in range(len(ps))], raw


def _law_cases():
    py = O.PyEC()
    pts = O.hash_points(b"chain", 260)
    G = (O.GX, O.GY)
    ps, qs = pts[:128], pts[128:256]                                  # random pairs
    ps += [None, G, None, pts[0], pts[1], G, pts[2], pts[256]]        # infinity on either side and both, P = Q, P = -Q
    qs += [G, None, None, pts[0], py.neg(pts[1]), G, py.neg(pts[2]), py.neg(pts[256])]
    return py, ps, qs


@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_chain_add_matches_plain_add(gpu, op):
    """op bit 0 / 1: the left / right operand is 3 P, a sum of three points with ZZ != 1.  With both bits set P = Q and P = -Q meet in
    XYZZ form on both sides; with one, 3 P against Q (different points) and against infinity."""
    py, ps, qs = _law_cases()
    got, raw = _chain_op(gpu, op, ps, qs)
    bad = [i for i in range(len(ps)) if not np.array_equal(raw[i, :40], raw[i, 40:])]
    assert not bad, f"chain and plain limbs differ at {bad[:8]}"
    t3 = lambda p: py.add(py.add(p, p), p)
    want = [py.add(t3(p) if op & 1 else p, t3(q) if op & 2 else q) for p, q in zip(ps, qs)]
    assert got == want


@pytest.mark.parametrize("op", [4, 5])
def test_chain_dbl_matches_plain_dbl(gpu, op):
    py, ps, _ = _law_cases()
    got, raw = _chain_op(gpu, op, ps, ps)
    bad = [i for i in range(len(ps)) if not np.array_equal(raw[i, :40], raw[i, 40:])]
    assert not bad, f"chain and plain limbs differ at {bad[:8]}"
    t3 = lambda p: py.add(py.add(p, p), p)
    assert got == [py.add(t3(p), t3(p)) if op & 1 else py.add(p, p) for p in ps]


@pytest.mark.parametrize("op", [4, 5, 6, 7])
def test_quad_forms_on_the_lone_multiplier(gpu, op):
    """xyzz_add_quad / xyzz_dbl_quad on fq_mul_lone (one product per lane on a lone wavefront: k_reduce_tail_quad) against xyzz_add /
    xyzz_dbl limb for limb, on the cases of the group-law tests; op 5 / 7: inputs at the magnitude bounds (bppp_test_point_quad)."""
    py, ps, qs = _law_cases()
    dbl = (op & 3) >= 2
    if dbl:
        qs = ps
    A, B = points_to_array(ps), points_to_array(qs)
    out = np.zeros_like(A)
    raw = np.zeros((len(ps), 81), dtype=np.uint32)
    rc = load_test_library().bppp_test_point_quad(gpu.h, op, A.ctypes.data, B.ctypes.data, len(ps), out.ctypes.data, raw.ctypes.data)
    assert rc == 0, gpu.lib.bppp_last_error(gpu.h)
    bad = [i for i in range(len(ps)) if not np.array_equal(raw[i, :40], raw[i, 40:80])]
    assert not bad, f"quad and one-lane limbs differ at {bad[:8]}"
    assert raw[:, 80].all()
    assert [array_to_point(out[i]) for i in range(len(ps))] == [py.add(p, q) for p, q in zip(ps, qs)]


# ---- pipeline
@pytest.fixture(scope="module")
def ctxs(gpu):
    """the contexts the pipeline cases run on: the default one (the quad tail; the one-lane tail it was once compared with is gone)"""
    return [gpu]


def _hook(g, name):
    v = ctypes.c_int(-2)
    assert getattr(load_test_library(), name)(g.h, ctypes.byref(v)) == 0
    return v.value


def _msm_both(ctxs, sc, pts, c):
    sa, pa = scalars_to_array(sc), points_to_array(pts)
    out = []
    for g in ctxs:
        ds, dp = g.to_device(sa), g.to_device(pa)
        try:
            out.append(g.msm_device(ds, dp, len(sc), window_bits=c))
        finally:
            g.free(ds); g.free(dp)
        # the route: whole buckets by size and the ranged scatter at 16 bits only; windows as csrc/msm.hip window_layout gives them
        assert _hook(g, "bppp_test_last_acc_sized") == (1 if c == 16 else 0)
        assert _hook(g, "bppp_test_last_windows") == {9: 29, 12: 22, 13: 20, 16: 16}[c]
        assert (_hook(g, "bppp_test_last_sort_ranges") > 0) == (c == 16)
    return out[0]


@pytest.fixture(scope="module")
def random_case(oracle_lib):
    n = 4096
    rnd = random.Random(1104)
    pts = O.hash_points(b"chain msm", n)
    sc = [rnd.randrange(O.N) for _ in range(n)]
    for i in range(0, n, 13):
        sc[i] = 0
    return sc, pts, oracle_lib.inner_product(list(zip(sc, pts)))


@pytest.mark.parametrize("c", [9, 12, 16])
def test_marginal_sums_and_both_tails(ctxs, random_case, c):
    """n = 4096: M = 256, 2048 and 32768 buckets per window, i.e. (HI, LO) = (16, 16), (32, 64) and (128, 256)"""
    sc, pts, want = random_case
    assert _msm_both(ctxs, sc, pts, c) == want


@pytest.mark.parametrize("c", [13, 16])
def test_heavy_bucket(ctxs, oracle_lib, c):
    """n = 40 000 with 39 000 scalars equal: one bucket per window takes nearly everything — k_merge_heavy over the lanes' partial sums
    (13 bits) or over 305 piece sums, two chunks and the last arriver's join (16 bits).  The points are 256 distinct ones repeated, so the
    oracle sums 256 terms."""
    n, m = 40000, 256
    rnd = random.Random(1105)
    base = O.hash_points(b"chain heavy", m)
    a = rnd.randrange(O.N)
    sc = [a] * 39000 + [rnd.randrange(O.N) for _ in range(n - 39000)]
    rnd.shuffle(sc)
    tot = [0] * m
    for i, s in enumerate(sc):
        tot[i % m] = (tot[i % m] + s) % O.N
    want = oracle_lib.inner_product(list(zip(tot, base)))
    assert _msm_both(ctxs, sc, [base[i % m] for i in range(n)], c) == want


@pytest.mark.parametrize("c", [9, 12, 16])
def test_equal_points_meet_in_the_reduce_trees(ctxs, c):
    """All scalars 1 and all points equal: one bucket, everything else infinity.  Then scalars 1 .. 4 over one point: the four buckets hold
    the same sum, so the serial loop of k_reduce_marg, its tree and the tails add P to P (the doubling branch of the chain addition)."""
    py = O.PyEC()
    G = (O.GX, O.GY)
    n = 4096
    assert _msm_both(ctxs, [1] * n, [G] * n, c) == py.mul(n, G)
    assert _msm_both(ctxs, [1, 2, 3, 4] * (n // 4), [G] * n, c) == py.mul(10 * (n // 4), G)


@pytest.mark.parametrize("s", [1, 2, 4])
def test_serial_lengths_of_the_prefetching_loop(random_case, s, monkeypatch):
    """The serial sum of k_reduce_marg loads bucket k + 1 before it adds bucket k.  BPPP_MARG_S (read when a context is made) sets its length:
    1 (nothing to add), 2 (one addition, no loop) and 4 (the loop); the plan's own choice at these sizes is 1, and 16 at 16-bit windows."""
    import bulletproofspp_amd as b
    sc, pts, want = random_case
    monkeypatch.setenv("BPPP_MARG_S", str(s))
    g = b.Bppp(0)
    try:
        ds, dp = g.to_device(scalars_to_array(sc)), g.to_device(points_to_array(pts))
        try:
            assert g.msm_device(ds, dp, len(sc), window_bits=12) == want
        finally:
            g.free(ds); g.free(dp)
    finally:
        g.close()
