"""The mixed additions of the bucket accumulation - xyzz_madd (csrc/ec.hip.h, 10 x 26-bit limbs) and xyzz29_madd (csrc/ec29.hip.h, 9 x 29) - on the
inputs where they must DECIDE: the point that comes in equals, or is opposite to, the accumulator while the accumulator holds a SUM (ZZ != 1, X up
to magnitude 5, Y up to 3), or shares only its y with it.  Both routines settle P = +-Q by a zero test on a lazily reduced difference; every other
test feeds them that case only on an accumulator just loaded from an affine point (ZZ = 1), and the whole-MSM tests use hashed points, which never
collide.  A verifier's MSM runs over points an attacker chooses: C = A + B in one bucket is an input like any other.

Chains through bppp_test_madd26_chain and bppp_test_madd29_chain (the first entry loaded, the others added, flags[j] negating entry j first: the walk
of k_acc_points_sized / k_acc_points_sized29 over an item) on points k G with k known, lambda-images of them (the same y, x times beta) and a few
hashed points.  The reference is the oracle's sum of the chain, entry by entry; where all logs are known it is checked against (sum k) G as well.
Both forms must equal it, hence each other; the stored sums keep what the readers of the bucket array rely on: every limb of the 29-bit form's
output below 2^26, ZZ all zero exactly for infinity.  Every launch has at least 70 chains: more than one wavefront."""
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd.capi import array_to_point, load_test_library, points_to_array

pytestmark = pytest.mark.gpu

N, P = O.N, O.P
G = (O.GX, O.GY)
CAP = 128                         # ACC_CAP of csrc/msm_plan.hpp
KMAX = 4096


class Curve:
    """k -> k G through the oracle: a table for |k| <= KMAX built by repeated addition, one scalar multiplication for any other log"""

    def __init__(self, ec):
        self.ec, self.tab, self.memo = ec, {0: None}, {}
        p = None
        for k in range(1, KMAX + 1):
            p = ec.add(p, G)
            self.tab[k], self.tab[-k] = p, ec.neg(p)
        assert self.tab[1] == G and self.tab[KMAX] == ec.mul(KMAX, G)

    def pt(self, k):
        if k in self.tab:
            return self.tab[k]
        k %= N
        if k not in self.memo:
            self.memo[k] = self.ec.mul(k, G) if k else None
        return self.memo[k]

    def beta(self, k, times=1):
        """the lambda-image of k G: the same y, x times beta (twice: beta^2), with its log"""
        x, y = self.pt(k)
        return (x * pow(O.BETA, times, P) % P, y), k * pow(O.LAMBDA, times, N) % N


@pytest.fixture(scope="module")
def curve(oracle_lib):
    cv = Curve(oracle_lib)
    assert oracle_lib.mul(O.LAMBDA, G) == (O.BETA * O.GX % P, O.GY)               # as test_group_law_complete
    for k in (1, 7, -KMAX):
        for t in (1, 2):
            q, lk = cv.beta(k, t)
            assert oracle_lib.on_curve(q) and q == oracle_lib.mul(lk, G) and q[0] != cv.pt(k)[0]
    return cv


@pytest.fixture(scope="module")
def hashed():
    return O.hash_points(b"madd collisions", 64)


def _run(gpu, fq29, chains):
    k, n = len(chains[0]), len(chains)
    assert all(len(c) == k for c in chains) and n >= 70
    parr = np.ascontiguousarray(points_to_array([p for c in chains for p, _ in c]))
    flags = np.ascontiguousarray(np.array([1 if s else 0 for c in chains for _, s in c], dtype=np.uint32))
    out = np.zeros((n, 8), dtype=np.uint64); raw = np.zeros((n, 40), dtype=np.uint32)
    lib = load_test_library()
    rc = (lib.bppp_test_madd29_chain if fq29 else lib.bppp_test_madd26_chain)(gpu.h, parr.ctypes.data, flags.ctypes.data, k, n, out.ctypes.data, raw.ctypes.data)
    assert rc == 0, gpu.lib.bppp_last_error(gpu.h)
    return out, raw


def _check(gpu, ec, curve, chains, logs=None):
    """chains: equally long lists of (point or None, negate); logs: per chain the log of its sum where every entry's is known (else None)"""
    want = []
    for i, c in enumerate(chains):
        acc = None
        for p, s in c:
            acc = ec.add(acc, ec.neg(p) if s else p)
        if logs is not None and logs[i] is not None:
            assert acc == curve.pt(logs[i]), ("the oracle's sum against (sum k) G", i)
        want.append(acc)
    o26, r26 = _run(gpu, False, chains)
    o29, r29 = _run(gpu, True, chains)
    assert (r29 < (1 << 26)).all()
    for i, w in enumerate(want):
        assert array_to_point(o26[i]) == w, ("10 x 26", len(chains[0]), i)
        assert array_to_point(o29[i]) == w, ("9 x 29", len(chains[0]), i)
        assert (not r26[i, 20:30].any()) == (w is None), ("10 x 26: ZZ all zero exactly for infinity", i)
        assert (not r29[i, 20:30].any()) == (w is None), ("9 x 29: ZZ all zero exactly for infinity", i)
    assert (o26 == o29).all()


def _small(rnd, avoid=()):
    while True:
        k = rnd.randrange(-KMAX // 4, KMAX // 4)
        if k and k not in avoid:
            return k


def _edge_logs(curve):
    """the k, |k| <= KMAX, whose k G has the smallest / largest x and y of the table"""
    ks = [k for k in curve.tab if k]
    pick = set()
    for coord in (0, 1):
        for f in (min, max):
            pick.add(f(ks, key=lambda k: curve.tab[k][coord]))
    pick |= {-k for k in pick}
    assert 4 <= len(pick) <= 8
    return sorted(pick)


def _collision_chains(curve, hashed, ec, rnd, extra):
    """chains of 2 + extra leading points whose sum S the accumulator holds (ZZ != 1) when the deciding entry comes in; returns {length: (chains, logs)}"""
    by_len = {}

    def put(chain, log):
        cs, ls = by_len.setdefault(len(chain), ([], []))
        cs.append(chain); ls.append(log)

    def family(lead, s, D):
        """lead: [(log, negate-through-the-flag)] summing to s"""
        S, nS = curve.pt(s), curve.pt(-s)
        head = [(curve.pt(-k if f else k), f) for k, f in lead]     # the flag negates the entry first: hand in -k G to add k G
        put(head + [(S, False)], 2 * s)                             # doubling at ZZ != 1
        put(head + [(nS, False)], 0)                                # cancellation at ZZ != 1
        put(head + [(nS, True)], 2 * s)                             # the same two through the sign fold
        put(head + [(S, True)], 0)
        put(head + [(S, False), (curve.pt(D), False)], 2 * s + D)   # going on after either
        put(head + [(nS, False), (curve.pt(D), False)], D)
        put(head + [(nS, True), (curve.pt(D), True)], 2 * s - D)
        for t in (1, 2):                                            # the same y, another x: R = 0 but Pd != 0
            q, lk = curve.beta(s, t)
            put(head + [(q, False)], s + lk)
            put(head + [(ec.neg(q), True)], s + lk)
            put(head + [(q, False), (S, False)], 2 * s + lk)
    for _ in range(12):
        lead = [(_small(rnd), rnd.random() < 0.3) for _ in range(2 + extra)]
        s = sum(k for k, _ in lead)
        if s == 0 or any(sum(k for k, _ in lead[:j]) == 0 for j in range(2, len(lead))):
            continue
        family(lead, s, _small(rnd, avoid=(s, -s, 2 * s, -2 * s)))
    # sums with an edge coordinate: S = k G for the k with the smallest and largest x and y of the table, split as A + B
    for k in _edge_logs(curve):
        done = 0
        while done < 2:
            parts = [_small(rnd) for _ in range(1 + extra)]
            parts.append(k - sum(parts))
            if any(x == 0 or abs(x) > KMAX for x in parts) or sum(parts[:2]) == 0:
                continue
            family([(x, False) for x in parts], k, _small(rnd, avoid=(k, -k, 2 * k, -2 * k)))
            done += 1
    # hashed points: no logs, the oracle's sum alone
    for i in range(0, 24, 2 + extra):
        hs = hashed[i:i + 2 + extra]
        S = None
        for h in hs:
            S = ec.add(S, h)
        head = [(h, False) for h in hs]
        put(head + [(S, False)], None); put(head + [(ec.neg(S), False)], None); put(head + [(ec.neg(S), True)], None)
        put(head + [((S[0] * O.BETA % P, S[1]), False)], None)
        put(head + [(S, False), (hashed[40 + i], False)], None); put(head + [(ec.neg(S), False), (hashed[40 + i], True)], None)
    return by_len


@pytest.mark.parametrize("extra", (0, 1))
def test_the_accumulator_holds_a_sum(gpu, oracle_lib, curve, hashed, extra):
    """[A, B, +-(A + B)], [A, B, C, +-(A + B + C)], on after either, through the sign fold, the lambda-image of the sum; sums with edge coordinates"""
    by_len = _collision_chains(curve, hashed, oracle_lib, random.Random(100 + extra), extra)
    assert sorted(by_len) == [3 + extra, 4 + extra]
    for k, (chains, logs) in sorted(by_len.items()):
        _check(gpu, oracle_lib, curve, chains, logs)


def test_same_y_right_after_the_load(gpu, oracle_lib, curve):
    """[A, (beta x_A, y_A)]: R = 0 and Pd != 0 on an accumulator with ZZ = 1, both signs, both non-trivial cube roots"""
    rnd = random.Random(7)
    chains, logs = [], []
    for _ in range(18):
        a = _small(rnd)
        for t in (1, 2):
            q, lk = curve.beta(a, t)
            chains += [[(curve.pt(a), False), (q, False)], [(curve.pt(-a), True), (oracle_lib.neg(q), True)]]
            logs += [a + lk, a + lk]
    _check(gpu, oracle_lib, curve, chains, logs)


def test_full_length_chains(gpu, oracle_lib, curve):
    """ACC_CAP entries, the last one equal or opposite to the sum of the 127 before it, directly and through the sign fold; then the lambda-image"""
    rnd = random.Random(128)
    chains, logs = [], []
    for i in range(72):
        while True:
            lead = [(_small(rnd), rnd.random() < 0.5) for _ in range(CAP - 1)]
            s = sum(k for k, _ in lead)
            if s:
                break
        head = [(curve.pt(-k if f else k), f) for k, f in lead]
        kind = i % 6
        if kind < 4:
            plus, fold = kind & 1, bool(kind & 2)                   # the entry adds +S or -S; handed in negated when it goes through the flag
            e = s if plus else -s
            chains.append(head + [(curve.pt(-e if fold else e), fold)]); logs.append(s + e)
        else:
            q, lk = curve.beta(s, kind - 3)
            chains.append(head + [(q, False)]); logs.append(s + lk)
    _check(gpu, oracle_lib, curve, chains, logs)
