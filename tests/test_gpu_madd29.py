"""Chains of mixed additions over 9 x 29-bit limbs (csrc/ec29.hip.h: xyzz29_madd, as k_acc_points_sized29 walks an item) through
bppp_test_madd29_chain, against the oracle's point sums: random chains of 1, 2, 3 and 128 points (ACC_CAP, the piece length), a doubling
inside a chain, P - P and on, infinity first / inside / last, 128 times one point, P and -P alternating.  The stored form of every sum keeps
the invariants the readers of the bucket array rely on: every limb below 2^26, ZZ all zero exactly for infinity."""
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd.capi import array_to_point, load_test_library, points_to_array

pytestmark = pytest.mark.gpu

CAP = 128                         # ACC_CAP of csrc/msm.hip


@pytest.fixture(scope="module")
def pts():
    return O.hash_points(b"madd29", 400)


def _chains(gpu, oracle_lib, chains):
    """chains: equally long lists of (point or None, negate); returns nothing, asserts every sum"""
    k, n = len(chains[0]), len(chains)
    assert all(len(c) == k for c in chains)
    parr = np.ascontiguousarray(points_to_array([p for c in chains for p, _ in c]))
    flags = np.ascontiguousarray(np.array([1 if s else 0 for c in chains for _, s in c], dtype=np.uint32))
    out = np.zeros((n, 8), dtype=np.uint64); raw = np.zeros((n, 40), dtype=np.uint32)
    rc = load_test_library().bppp_test_madd29_chain(gpu.h, parr.ctypes.data, flags.ctypes.data, k, n, out.ctypes.data, raw.ctypes.data)
    assert rc == 0, gpu.lib.bppp_last_error(gpu.h)
    assert (raw < (1 << 26)).all()
    for i, c in enumerate(chains):
        terms = [(O.N - 1 if s else 1, p) for p, s in c if p is not None]
        want = oracle_lib.inner_product(terms) if terms else None
        assert array_to_point(out[i]) == want, (k, i)
        assert (not raw[i, 20:30].any()) == (want is None), (k, i)


@pytest.mark.parametrize("k", (1, 2, 3, CAP))
def test_random_chains(gpu, oracle_lib, pts, k):
    rnd = random.Random(k)
    n = 70 if k < CAP else 3                     # more than a wavefront of short chains
    _chains(gpu, oracle_lib, [[(pts[rnd.randrange(len(pts))], rnd.random() < 0.5) for _ in range(k)] for _ in range(n)])


def test_special_chains_of_three(gpu, oracle_lib, pts):
    P, Q = pts[0], pts[1]
    _chains(gpu, oracle_lib, [
        [(P, False), (P, False), (Q, False)],            # doubling right after the load
        [(Q, False), (P, False), (P, False)],            # an ordinary sum, then P again: no doubling (Q + P != P)
        [(P, False), (P, True), (Q, False)],             # through infinity and on
        [(P, True), (P, True), (P, False)],              # the sign fold into the doubling: -2P + P
        [(None, False), (P, False), (Q, False)],         # infinity first
        [(P, False), (None, False), (Q, False)],         # ... in the middle
        [(P, False), (Q, False), (None, False)],         # ... last
        [(None, False), (None, True), (None, False)],    # ... alone
        [(P, False), (P, True), (None, False)],          # the sum is infinity
    ])


def test_special_chains_of_two_and_one(gpu, oracle_lib, pts):
    P = pts[2]
    _chains(gpu, oracle_lib, [[(P, False), (P, False)], [(P, False), (P, True)], [(None, False), (P, True)], [(P, True), (None, False)]])
    _chains(gpu, oracle_lib, [[(P, False)], [(P, True)], [(None, False)]])


def test_long_special_chains(gpu, oracle_lib, pts):
    P, rnd = pts[3], random.Random(9)
    same = [(P, False)] * CAP                                          # one doubling, then 126 additions of P to a multiple of P
    alt = [(P, bool(j & 1)) for j in range(CAP)]                       # P, -P, P, -P, ...: infinity after every second entry
    mixed = [(pts[rnd.randrange(len(pts))], rnd.random() < 0.5) for _ in range(CAP)]
    mixed[40] = (None, False); mixed[41] = mixed[39]; mixed[90] = (mixed[89][0], not mixed[89][1])
    _chains(gpu, oracle_lib, [same, alt, mixed, alt[1:] + [(P, False)]])
