"""The bit-exact model of csrc/fq29.hip.h and csrc/ec29.hip.h (benchmarks/fe29_model.py): its own 64 / 32-bit assertions at the worst-case
bounds of every routine, tight x loose-7 products with every limb at its maximum, 10^4 random pairs against Python integers mod p, and the
forbidden magnitude pairs, which must trip the overflow assertion (so the assertion is live).  No GPU."""
import importlib.util
import os
import random

import pytest

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "benchmarks", "fe29_model.py")
_spec = importlib.util.spec_from_file_location("fe29_model", _PATH)
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

P = M.P


def test_constants():
    assert M.val(M.PL) == P
    assert (M.R1 << 29) + M.R0 == (1 << 261) % P == 0x2000007A20
    assert M.mag_limbs(M.MAX_MAG)[0] < (1 << 32) <= M.mag_limbs(M.MAX_MAG + 1)[0]


def test_worst_case_bounds_of_every_routine():
    """upper-bound runs and exact runs on the largest limbs of each contract: mul, sqr, weak_pass, to_fq26, sub, the mixed addition with
    X = 5, Y = 3, ZZ = ZZZ = 1, y = 2, and the doubling"""
    M.check_bounds()


@pytest.mark.parametrize("ma,mb", [(1, 7), (7, 1)])
def test_tight_times_loose7_at_the_maxima(ma, mb):
    a, b = M.mag_limbs(ma), M.mag_limbs(mb)
    r = M.mul(a, b)
    assert M.mag_ok(r, 1) and M.val(r) % P == M.val(a) * M.val(b) % P
    M.mul(a, b, bound=True)
    # one limb at its maximum at a time, the others random: each column's largest single product
    rnd = random.Random(7)
    for i in range(9):
        for j in range(9):
            x, y = M.rand_mag(rnd, ma), M.rand_mag(rnd, mb)
            x[i], y[j] = M.mag_limbs(ma)[i], M.mag_limbs(mb)[j]
            assert M.val(M.mul(x, y)) % P == M.val(x) * M.val(y) % P


def test_squares_at_the_maxima():
    for m in (1, 2):
        a = M.mag_limbs(m)
        r = M.sqr(a)
        assert M.mag_ok(r, 1) and M.val(r) % P == M.val(a) ** 2 % P


def test_random_pairs_against_integers():
    rnd = random.Random(2929)
    for it in range(10000):
        ma = rnd.choice([1, 2, 3, 5, 7])
        mb = rnd.choice([m for m in [1, 2, 3, 5, 7] if m * ma <= 7])
        a, b = M.rand_mag(rnd, ma), M.rand_mag(rnd, mb)
        va, vb = M.val(a), M.val(b)
        r = M.mul(a, b)
        assert M.mag_ok(r, 1) and M.val(r) % P == va * vb % P
        if ma <= 2:
            s = M.sqr(a)
            assert M.mag_ok(s, 1) and M.val(s) % P == va * va % P
        if ma + mb + 1 <= M.MAX_MAG:
            d = M.sub(a, b, mb)
            assert M.mag_ok(d, ma + mb + 1) and M.val(d) % P == (va - vb) % P
            w = M.weak_pass(d)
            assert M.mag_ok(w, 1) and max(w[:8]) < (1 << 29) and M.val(w) % P == (va - vb) % P
        t = M.to_fq26(a)
        assert max(t) < (1 << 26) and sum(x << (26 * j) for j, x in enumerate(t)) % P == va % P


def test_canonical_values_round_trip():
    rnd = random.Random(3)
    for v in [0, 1, P - 1, P - 2**32, 2**256 - 1 - 2**32 - 977] + [rnd.randrange(P) for _ in range(500)]:
        words = [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
        a = M.from_fe(words)
        assert M.mag_ok(a, 1) and M.val(a) == v
        assert sum(x << (26 * j) for j, x in enumerate(M.to_fq26(a))) == v


def test_zero_test():
    for k in range(4):
        assert M.normalizes_to_zero([k * x for x in M.PL])
    assert M.normalizes_to_zero(M.sub(M.from_int(5), M.from_int(5), 1))
    assert M.normalizes_to_zero(M.sub(M.mag_limbs(1), M.mag_limbs(1), 5))
    for v in (1, P - 1, P + 1, 2 * P - 1, 2**256):
        assert not M.normalizes_to_zero(M.from_int(v))


def test_forbidden_pairs_trip_the_overflow_assertion():
    M.forbidden_pairs_trip()
    for ma, mb in [(1, 8), (2, 4)]:
        a = M.mag_limbs(ma)
        b = [min(v, (1 << 32) - 1) for v in M.mag_limbs(mb)]
        with pytest.raises(M.Overflow):
            M.mul(a, b)
        with pytest.raises(M.Overflow):
            M.mul(a, b, bound=True)
    with pytest.raises(M.Overflow):
        M.sqr(M.mag_limbs(3))
    with pytest.raises(M.Overflow):
        M.sub(M.mag_limbs(1), M.mag_limbs(4), 3)      # a subtrahend above the declared magnitude


def test_mixed_addition_chains_against_integers():
    """random points, P + P, P - P, infinity inside the chain, the sign fold on y"""
    rnd = random.Random(2008)
    for it in range(12):
        pts = [M.rand_point(rnd) for _ in range(5)]
        neg = lambda p: (p[0], P - p[1])
        chain = [pts[0], pts[1], pts[1], None, neg(pts[2]), pts[2], pts[2], pts[3], pts[4], neg(pts[4])]
        if it % 3 == 1:
            chain = [None, pts[0], pts[0], neg(pts[0]), neg(pts[0]), pts[1], None]
        acc, ref = M.xyzz_inf(), None
        for pt in chain:
            q = [M.from_int(0), M.from_int(0)] if pt is None else [M.from_int(pt[0]), M.from_int(pt[1])]
            if pt is not None and rnd.random() < 0.5:
                q[1] = M.neg(M.from_int(P - pt[1]), 1)
            acc = M.xyzz_madd(acc, q)
            ref = M.ec_add(ref, pt)
            assert M.xyzz_affine(acc) == ref
            stored = [M.to_fq26(c) for c in acc]
            assert all(max(c) < (1 << 26) for c in stored) and (not any(stored[2])) == (ref is None)
