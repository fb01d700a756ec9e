"""The routines of the exception-free sized accumulation (csrc/fq29.hip.h: fq29_mul_add2; csrc/ec29.hip.h: xyzz29_madd_fast, xyzz29_from_two) through
bppp_test_ec29_fast_op, on raw limbs built here: every result equals the bit-exact model (benchmarks/fe29_model.py) limb for limb, and the integers
by value.  mul_add2 at tight operands, at every worst case of its contract (magnitude products adding up to 7) and at random limbs inside it;
madd_fast on a few hundred seeded points with either sign fold, on accumulators that a chain of the model left behind (its own, and the complete
addition's with Y of magnitude 3), at the largest limbs of its magnitudes, and on the inputs it is not made for (P = +-Q): ZZ = 0 (mod p) comes
back, and stays; from_two on 300 seeded pairs, on x1 = x2 and at its largest limbs.  The one-call kernel does not show the compiler's dropped
mask on limb 8 (ec29.hip.h): its operands come from memory; tests/test_gpu_msm_acc_fast.py runs the routines where it appeared."""
import importlib.util
import os
import random

import numpy as np
import pytest

from bulletproofspp_amd.capi import load_test_library

pytestmark = pytest.mark.gpu

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "benchmarks", "fe29_model.py")
_spec = importlib.util.spec_from_file_location("fe29_model", _PATH)
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

P = M.P
OPS = {"mul_add2": 0, "madd_fast": 1, "from_two": 2}


def _run(gpu, op, rows):
    """rows: per case the list of field elements (9 limbs each) the op takes; returns per case the 4 x 9 result limbs"""
    arr = np.ascontiguousarray(np.array(rows, dtype=np.uint32).reshape(len(rows), -1))
    assert arr.shape[1] == (54 if op == "madd_fast" else 36)
    raw = np.zeros((len(rows), 36), dtype=np.uint32)
    rc = load_test_library().bppp_test_ec29_fast_op(gpu.h, OPS[op], arr.ctypes.data, len(rows), raw.ctypes.data)
    assert rc == 0, gpu.lib.bppp_last_error(gpu.h)
    return [[[int(x) for x in r[9 * j:9 * j + 9]] for j in range(4)] for r in raw]


def _aff(rnd, pt):
    """(x, y) limbs of a point, y through the sign fold (2 p - (p - y), magnitude 2) half of the time"""
    y = M.neg(M.from_int(P - pt[1]), 1) if rnd.random() < 0.5 else M.from_int(pt[1])
    return [M.from_int(pt[0]), y]


def test_mul_add2_against_the_model(gpu):
    rnd = random.Random(292)
    edge = [M.from_int(v) for v in (0, 1, 2, P - 1, P - 2**32, 977, 2**255, 2**256 - 1)] + [[M.M29] * 8 + [M.M24], M.mag_limbs(1), M.PL]
    rows = [[M.from_int(rnd.randrange(P)) for _ in range(4)] for _ in range(1024)]
    for x in edge:
        for y in edge:
            rows += [[x, y, y, x], [x, x, y, y], [x, y, M.from_int(rnd.randrange(P)), M.from_int(rnd.randrange(P))]]
    for mags in M.MUL_ADD2_WORST + [(1, 1, 4, 1), (1, 1, 3, 1)]:
        rows.append([M.mag_limbs(m) for m in mags])                          # every limb at the largest value of its magnitude
        rows += [[M.rand_mag(rnd, m) for m in mags] for _ in range(48)]
    got = _run(gpu, "mul_add2", rows)
    for i, (a, b, c, d) in enumerate(rows):
        want = M.mul_add2(a, b, c, d)
        assert got[i][0] == want, i
        assert M.val(want) % P == (M.val(a) * M.val(b) + M.val(c) * M.val(d)) % P
        assert M.mag_ok(want, 1)


@pytest.fixture(scope="module")
def points():
    rnd = random.Random(2008)
    return [M.rand_point(rnd) for _ in range(64)]


def test_from_two_against_the_model(gpu, points):
    rnd = random.Random(21)
    rows, pairs = [], []
    for _ in range(300):
        p, q = rnd.sample(points, 2)
        rows.append(_aff(rnd, p) + _aff(rnd, q)); pairs.append((p, q))
    for p in points[:8]:                                                     # x1 = x2: P = Q and P = -Q, the inputs it is not made for
        rows.append(_aff(rnd, p) + _aff(rnd, p)); pairs.append(None)
        rows.append(_aff(rnd, p) + _aff(rnd, (p[0], P - p[1]))); pairs.append(None)
    rows.append([M.mag_limbs(1), M.mag_limbs(2), M.mag_limbs(1), M.mag_limbs(2)]); pairs.append(())
    got = _run(gpu, "from_two", rows)
    for i, r in enumerate(rows):
        assert got[i] == M.xyzz_from_two(r[:2], r[2:]), i
        if pairs[i] is None:
            assert M.normalizes_to_zero(got[i][2]) and M.normalizes_to_zero(got[i][3])
        elif pairs[i]:
            assert M.xyzz_affine(got[i]) == M.ec_add(*pairs[i]) and not M.normalizes_to_zero(got[i][2])


def test_madd_fast_against_the_model(gpu, points):
    rnd = random.Random(22)
    rows, refs = [], []
    for it in range(300):
        chain = rnd.sample(points, 1 + it % 6)                               # the accumulator: a loaded point and 0 .. 5 additions
        acc = M.xyzz_from_aff(_aff(rnd, chain[0]))
        ref = chain[0]
        for pt in chain[1:]:
            acc = M.xyzz_madd_fast(acc, _aff(rnd, pt)); ref = M.ec_add(ref, pt)
        q = rnd.choice([pt for pt in points if pt not in chain])
        rows.append(acc + _aff(rnd, q)); refs.append(M.ec_add(ref, q))
    for it in range(32):                                                     # the accumulator of the complete addition: Y of magnitude 3
        a, b, q = rnd.sample(points, 3)
        acc = M.xyzz_madd(M.xyzz_from_aff(_aff(rnd, a)), _aff(rnd, b))
        rows.append(acc + _aff(rnd, q)); refs.append(M.ec_add(M.ec_add(a, b), q))
    for p in points[:8]:                                                     # acc = 2 P + ... met by its own sum: P = Q, P = -Q; then a lane gone wrong goes on
        a, b = points[20], points[21]
        s = M.ec_add(a, b)
        acc = M.xyzz_madd_fast(M.xyzz_from_aff(_aff(rnd, a)), _aff(rnd, b))
        rows.append(acc + _aff(rnd, s)); refs.append(None)
        rows.append(acc + _aff(rnd, (s[0], P - s[1]))); refs.append(None)
        rows.append(M.xyzz_madd_fast(acc, _aff(rnd, s)) + _aff(rnd, p)); refs.append(None)
    rows.append([M.mag_limbs(5), M.mag_limbs(3), M.mag_limbs(1), M.mag_limbs(1), M.mag_limbs(1), M.mag_limbs(2)]); refs.append(())
    got = _run(gpu, "madd_fast", rows)
    for i, r in enumerate(rows):
        want = M.xyzz_madd_fast(r[:4], r[4:])
        assert got[i] == want, i
        assert M.mag_ok(got[i][0], 5) and all(M.mag_ok(got[i][j], 1) for j in (1, 2, 3))
        if refs[i] is None:
            assert M.normalizes_to_zero(got[i][2])
        elif refs[i]:
            assert M.xyzz_affine(got[i]) == refs[i]
            assert not M.normalizes_to_zero(got[i][2])
