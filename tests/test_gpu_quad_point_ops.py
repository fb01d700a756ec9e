"""The quad point operations (csrc/ec_quad.hip.h: four lanes share one XYZZ addition or doubling) against the one-lane forms of
csrc/ec.hip.h, raw 26-bit limbs bit for bit, and both against the oracle; then the MSM's bucket-reduction tail on quads against the
one-lane tail it replaces."""
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd.capi import array_to_point, load_test_library, points_to_array, scalars_to_array

pytestmark = pytest.mark.gpu


def _quad_op(gpu, op, ps, qs):
    A, B = points_to_array(ps), points_to_array(qs)
    out = np.zeros_like(A)
    raw = np.zeros((len(ps), 81), dtype=np.uint32)
    lib = load_test_library()
    rc = lib.bppp_test_point_quad(gpu.h, op, A.ctypes.data, B.ctypes.data, len(ps), out.ctypes.data, raw.ctypes.data)
    assert rc == 0, gpu.lib.bppp_last_error(gpu.h)
    return [array_to_point(out[i]) for i in range(len(ps))], raw


def _check(gpu, op, ps, qs, want):
    got, raw = _quad_op(gpu, op, ps, qs)
    bad = [i for i in range(len(ps)) if not np.array_equal(raw[i, :40], raw[i, 40:80])]
    assert not bad, f"quad and scalar limbs differ at {bad[:8]}"
    assert raw[:, 80].all(), f"lanes of a quad disagree at {np.flatnonzero(raw[:, 80] == 0)[:8].tolist()}"
    assert got == want


def _cases():
    py = O.PyEC()
    pts = O.hash_points(b"quad", 400)
    G = (O.GX, O.GY)
    ps, qs = pts[:200], pts[200:]                                    # random pairs
    ps += [None, G, None, pts[0], pts[1], G, pts[2]]                 # infinity on either side, P = Q, P = -Q
    qs += [G, None, None, pts[0], py.neg(pts[1]), G, py.neg(pts[2])]
    # one wavefront (16 quads, from a multiple of 16) whose quads take every branch of the complete law side by side
    while len(ps) % 16:
        ps.append(pts[len(ps) % 50]); qs.append(pts[399 - len(ps) % 50])
    for k in range(16):
        p = pts[300 + k]
        q = [pts[350 + k], p, py.neg(p), None, pts[380 + (k % 10)]][k % 5]
        ps.append(None if k % 7 == 3 else p); qs.append(q)
    return py, ps, qs


@pytest.mark.parametrize("bounds", [0, 1])
def test_quad_add_matches_scalar_add(gpu, bounds):
    py, ps, qs = _cases()
    _check(gpu, bounds, ps, qs, [py.add(p, q) for p, q in zip(ps, qs)])


@pytest.mark.parametrize("bounds", [0, 1])
def test_quad_dbl_matches_scalar_dbl(gpu, bounds):
    py, ps, _ = _cases()
    _check(gpu, 2 + bounds, ps, ps, [py.add(p, p) for p in ps])


def _msm_case(n, seed):
    rnd = random.Random(seed)
    pts = O.hash_points(b"qtail%d" % seed, n)
    sc = [rnd.randrange(O.N) for _ in range(n)]
    for i in range(0, n, 13):
        sc[i] = 0
    return sc, pts


@pytest.mark.parametrize("c", [9, 10, 12, 14, 16])
def test_quad_tail_equals_scalar_tail(gpu, oracle_lib, c):
    """Every (HI, LO) split of the marginal-sum reduction from 16 x 16 to 128 x 256: the quad tail gives the oracle's point, on random
    scalars and on one-bucket inputs.  (The one-lane tail it was once run beside has been removed.)"""
    G = (O.GX, O.GY)
    cases = [_msm_case(700, c), ([5] * 64 + [O.N - 5] * 63, [G] * 127), ([2**200 + 3] * 40, O.hash_points(b"one", 40))]
    for sc, pts in cases:
        want = oracle_lib.inner_product(list(zip(sc, pts)))
        ds, dp = gpu.to_device(scalars_to_array(sc)), gpu.to_device(points_to_array(pts))
        try:
            assert gpu.msm_device(ds, dp, len(sc), window_bits=c) == want
        finally:
            gpu.free(ds); gpu.free(dp)
