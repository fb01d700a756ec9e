"""Sealed outputs on the host, no GPU: rangeproof.seal_host / scan_host round trips over the oracle backend on rec_test and bin_test (3 ranges
each); r A == a R on the oracle; and a lane-for-lane replay of the fixed-scalar walk of csrc/rpseal.hip.h on integers mod n.

The replay takes points as discrete logs (P = k G is the integer k, infinity is 0) and follows the kernel step by step from the recoding the
library itself makes on the host (bppp_test_rp_scan_recode, compared here with oracle.decompose_eis): T1 = +-P, T2 = +-lambda P, T3 = T1 + T2,
one doubling per digit from the highest down and one addition per non-zero digit.  Every addition is classified the way the complete law
branches:
    table-infinity   the table point is infinity (P is): the addition returns at once
    infinity+point   the accumulator is infinity: it becomes the table point
    doubling         the accumulator equals the table point
    cancelling       the accumulator is the table point's negative
    general          none of these
Which of them can a walk reach?  Write a pair of signed halves (u, v) for u + v lambda and norm (u, v) = u^2 - u v + v^2 (the Eisenstein norm:
lambda is a cube root of unity mod n).  The pairs that are 0 mod n form the lattice of multiples of conj (charEis), whose norm is n: every
non-zero lattice vector has norm >= n.  The split subtracts a NEAR multiple, not the nearest: its quotient estimate (a shift by 256 bits for a
division by n) lies below the true quotient by up to 2.15 and ONE step corrects it by one, so the halves a are (e0 + e1 w) times that generator
with e0, e1 in (-0.5, 1.15]: norm (a) <= 2.2 n (n - 1 splits into halves of norm n; 10^5 random scalars reach 2.0 n).  All that is needed below
is norm (a) < 3.9 n, which replay asserts for every scalar it walks.  Before the addition of digit i the accumulator is 2 (a >> (i + 1)) (shifts on
the magnitudes) and the table point is the digit's, d; after it, a >> i.  `cancelling` needs a >> i, `doubling` needs 2 (a >> (i + 1)) - d, to be
zero or a non-zero lattice vector.  Zero: a >> i is zero only before the first addition (that is infinity+point), and 2 p = d for a digit d
means p = d = 0.  A lattice vector, i >= 1: a >> i is a / 2^i up to less than one unit a half, and 2 (a >> (i + 1)) - d lies within two units of
it, so both have norm below 3.9 n / 4 plus a few times 2^130 — below n (replay asserts both at every such step).  A lattice vector, i = 0: a itself
is one only for the scalar 0, whose split is (0, 0) and has no digit; a - 2 d is one only for the scalars 2 d = +-2, +-2 lambda, +-2 +- 2 lambda.
All of these but -2 split into those small pairs themselves, so that a - 2 d = 0 and there is no addition at digit 0; -2 = n - 2 splits into a long
pair whose digit 0 is not (-1, 0), so that its a - 2 d is no lattice vector (both in test_recoding_equals_the_librarys; n - 2 is walked too).  So
for a point of prime order the classes a walk can reach are infinity+point and general, plus table-infinity for P at infinity.
test_walk_replay_reaches_every_class asserts that WALK_SCALARS (the list tests/test_gpu_scan_walk.py runs on the GPU) reaches exactly those
three, with P = infinity among the GPU test's points, and that 2000 seeded scalars find no other either.
The two unreachable branches stay in the kernel because it uses the library's one complete law; tests/test_gpu_excess.py and
tests/test_gpu_excess_part.py cover them on crafted input."""
import collections
import ctypes as C
import hashlib
import json
import os
import random

import numpy as np

import pyoracle as O
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from rp_backends import OracleBackend
from test_rangeproof import EXAMPLES

N = O.N
LAMBDA = O.LAMBDA
TAG = b"seal tag"


def from_halves(h1, h2):
    return (h1 + h2 * LAMBDA) % N


# the halves the named scalars are put together from: runs of the maximal digit, alternating digits, long runs of zero digits
MAXIMAL = (2**125 - 1, 2**125 - 1)
ALT_12 = (int("01" * 62, 2), int("10" * 62, 2))
ALT_30 = (int("01" * 62, 2), int("01" * 62, 2))
ZERO_RUNS = (2**124 + 1, 2**123 + 2**61)
BOTH_NEGATIVE = [(-(2**100) - 3, -(2**90) - 5), (-(2**123) - 12345, -(2**123) + 99)]


def walk_scalars():
    """the scalars tests/test_gpu_scan_walk.py walks on the GPU; test_walk_replay_reaches_every_class replays the same list"""
    rng = random.Random(20)
    named = [1, 2, N - 2, N - 1, N, N + 1, 2**255, 2**256 - 1]
    named += [from_halves(*h) for h in (MAXIMAL, ALT_12, ALT_30, ZERO_RUNS)]
    named += [LAMBDA, LAMBDA + 1, LAMBDA - 1] + [from_halves(*h) for h in BOTH_NEGATIVE]
    return named + [rng.randrange(2**256) for _ in range(8)]


WALK_SCALARS = walk_scalars()
POINT_LOGS = [1, N - 1, 2, 3, 5, 7, 11, 0]              # G, -G, k G for small k, and infinity


def py_recode(x):
    """the recoding of csrc/rpseal.hip.h restated: (digits from digit 0 up, sign bits)"""
    a, b = O.decompose_eis(x % N)
    assert (a + b * LAMBDA - x) % N == 0
    nbits = max(abs(a).bit_length(), abs(b).bit_length())
    return [((abs(a) >> i) & 1) | (((abs(b) >> i) & 1) << 1) for i in range(nbits)], (1 if a < 0 else 0) | (2 if b < 0 else 0)


def lib_recode(x):
    tl = capi.load_test_library()
    s, out = capi.int_to_limbs(x), np.zeros(11, dtype=np.uint32)
    assert tl.bppp_test_rp_scan_recode(C.c_void_p(s.ctypes.data), C.c_void_p(out.ctypes.data)) == 0
    nbits = int(out[9])
    return [(int(out[i >> 4]) >> (2 * (i & 15))) & 3 for i in range(nbits)], int(out[10])


def replay(x, k):
    """(x k mod n as the walk computes it, the classes of its additions) for P = k G"""
    digits, neg = py_recode(x)
    classes = collections.Counter()

    def add(acc, t):
        cls = "table-infinity" if t == 0 else "infinity+point" if acc == 0 else "doubling" if acc == t else "cancelling" if (acc + t) % N == 0 else "general"
        classes[cls] += 1
        return (acc + t) % N
    t1 = (-k if neg & 1 else k) % N
    t2 = (-k if neg & 2 else k) * LAMBDA % N
    t3 = (t1 + t2) % N
    assert k == 0 or (t1 != t2 and (t1 + t2) % N != 0)                      # T3 is a general addition: lambda P is never +-P
    a = O.decompose_eis(x % N)
    sg = [-1 if h < 0 else 1 for h in a]
    norm = lambda u, v: u * u - u * v + v * v
    assert 10 * norm(*a) < 39 * N
    acc = 0
    for i in range(len(digits) - 1, -1, -1):
        acc = 2 * acc % N
        if digits[i]:
            after = [s * (abs(h) >> i) for s, h in zip(sg, a)]               # a >> i, and 2 (a >> (i + 1)) - d before it
            before = [s * (2 * (abs(h) >> (i + 1)) - ((digits[i] >> j) & 1)) for j, (s, h) in enumerate(zip(sg, a))]
            assert i == 0 or (norm(*after) < N and norm(*before) < N)
            assert (before[0] + before[1] * LAMBDA) * k % N == (acc - (t1, t2, t3)[digits[i] - 1]) % N
            acc = add(acc, (t1, t2, t3)[digits[i] - 1])
    return acc, classes


def _setups(oracle_lib):
    be = OracleBackend(oracle_lib)
    typed = RP.setup_from_schema(be, json.load(open(os.path.join(EXAMPLES, "rec_test", "schema.json"))))
    binary = BRP.setup_from_schema(be, json.load(open(os.path.join(EXAMPLES, "bin_test", "schema.json"))))
    return be, typed, binary


def test_round_trip_on_the_host(oracle_lib):
    ec = oracle_lib
    be, typed, binary = _setups(oracle_lib)
    rng = random.Random(3)
    for st in (typed, binary):
        g, H0, B = RP._excess_bases(st)
        nr = len(st.rds)
        assert nr == 3
        a, other = rng.randrange(1, N), rng.randrange(1, N)
        A = RP.excess_key33(ec.mul(a, B))
        r = rng.randrange(1, N)
        outputs = [(rng.randrange(2**32), rng.randrange(N) if H0 is not None else 0) for _ in range(nr)]
        outputs[1] = (-5, outputs[1][1])                                   # a negative amount reads back as n - 5
        status, seal, blinds = RP.seal_host(be, st, A, r, outputs, TAG)
        assert status == RP.SEAL_OK and len(seal) == RP.SEAL_BYTES(nr) and seal[:33] == RP.excess_key33(ec.mul(r, B))
        coms = [ec.inner_product([(v % N, g), (bl, B)] + ([(ty, H0)] if H0 is not None else [])) for (v, ty), bl in zip(outputs, blinds)]
        from bulletproofspp_amd import encoding
        file = encoding.encode_commitments(coms)
        want = [(v % N, ty, bl) for (v, ty), bl in zip(outputs, blinds)]
        assert RP.scan_host(be, st, a, file, seal, TAG) == (RP.SCAN_OWNED, want)
        zeros = [(0, 0, 0)] * nr
        verdict, opening = RP.scan_host(be, st, other, file, seal, TAG)
        assert verdict in (RP.SCAN_FOREIGN, RP.SCAN_TAG_ONLY) and opening == zeros
        assert RP.scan_host(be, st, a, file, seal, b"another tag")[0] != RP.SCAN_OWNED
        flipped = bytearray(seal)
        flipped[34 + 64 + 31] ^= 1                                           # a memo bit of range 1: the amount changes, the commitment no longer opens
        assert RP.scan_host(be, st, a, file, bytes(flipped), TAG) == (RP.SCAN_TAG_ONLY, zeros)
        assert RP.scan_host(be, st, a, file, seal[:32] + b"\x02" + seal[33:], TAG) == (RP.SCAN_BAD_HINT, zeros)
        swapped = encoding.encode_commitments([coms[1], coms[0], coms[2]])
        assert RP.scan_host(be, st, a, swapped, seal, TAG) == (RP.SCAN_TAG_ONLY, zeros)
        # refusals, the first that applies
        refused = lambda s: (s, bytes(RP.SEAL_BYTES(nr)), [0] * nr)
        assert RP.seal_host(be, st, A[:32] + b"\x02", 0, outputs, TAG) == refused(RP.EXCESS_BAD_KEY)
        assert RP.seal_host(be, st, A, N, outputs, TAG) == refused(RP.SEAL_NOT_CANONICAL)
        assert RP.seal_host(be, st, A, 0, outputs, TAG) == refused(RP.SEAL_ZERO)
        if H0 is not None:
            assert RP.seal_host(be, st, A, 0, [(1, N)] + outputs[1:], TAG) == refused(RP.SEAL_NOT_CANONICAL)
        # every message laid out by hand
        P = ec.mul(r, ec.mul(a, B))
        ss = hashlib.sha256(hashlib.sha256(b"bppp/seal/shared/v1" + TAG).digest() + RP._put(P[0]) + bytes([1 if P[1] > RP.FIELD_P - P[1] else 0]) + seal[:33]).digest()
        assert seal[33] == hashlib.sha256(hashlib.sha256(b"bppp/seal/tag/v1" + TAG).digest() + ss).digest()[0]
        for i in range(nr):
            le = bytes([i, 0, 0, 0])
            assert blinds[i] == RP.decode_field(hashlib.sha256(hashlib.sha256(b"bppp/seal/blind/v1" + TAG).digest() + ss + le).digest(), N)
            dm = hashlib.sha256(b"bppp/seal/memo/v1" + TAG).digest()
            pad = hashlib.sha256(dm + ss + le + b"\x00").digest() + hashlib.sha256(dm + ss + le + b"\x01").digest()
            plain = RP._put(outputs[i][0] % N) + RP._put(outputs[i][1])
            assert seal[34 + 64 * i:98 + 64 * i] == bytes(p ^ q for p, q in zip(plain, pad))


def test_shared_point_is_the_same_from_both_sides(oracle_lib):
    ec = oracle_lib
    _, typed, binary = _setups(oracle_lib)
    rng = random.Random(4)
    for st in (typed, binary):
        B = RP._excess_bases(st)[2]
        for _ in range(4):
            a, r = rng.randrange(1, N), rng.randrange(1, N)
            assert ec.mul(r, ec.mul(a, B)) == ec.mul(a, ec.mul(r, B))


def test_recoding_equals_the_librarys():
    rng = random.Random(21)
    for x in WALK_SCALARS + [0, N - 2, 3] + [rng.randrange(2**256) for _ in range(64)]:
        assert py_recode(x) == lib_recode(x), hex(x)
    # the named scalars have the digits they are named for
    assert O.decompose_eis(from_halves(*MAXIMAL)) == MAXIMAL and py_recode(from_halves(*MAXIMAL))[0] == [3] * 125
    assert py_recode(from_halves(*ALT_12))[0] == [1, 2] * 62 and py_recode(from_halves(*ALT_30))[0] == ([3, 0] * 62)[:-1]
    zr = py_recode(from_halves(*ZERO_RUNS))[0]
    assert zr.count(0) >= 119 and zr[62:123] == [0] * 61
    for h in BOTH_NEGATIVE:
        assert O.decompose_eis(from_halves(*h)) == h and py_recode(from_halves(*h))[1] == 3
    assert O.decompose_eis(LAMBDA) == (0, 1) and O.decompose_eis(LAMBDA + 1) == (1, 1) and O.decompose_eis(LAMBDA - 1) == (-1, 1)
    assert py_recode(N) == ([], 0) and py_recode(0) == ([], 0)
    for d1 in (-1, 0, 1):                                                    # the scalars 2 d: no addition at digit 0 can be a doubling
        for d2 in (-1, 0, 1):
            a = O.decompose_eis((2 * d1 + 2 * d2 * LAMBDA) % N)
            low = tuple((-1 if h < 0 else 1) * (abs(h) & 1) for h in a)
            assert a == (2 * d1, 2 * d2) or ((d1, d2) == (-1, 0) and low != (d1, d2))
    signs = {py_recode(x)[1] for x in WALK_SCALARS}
    assert signs == {0, 1, 2, 3}                                             # every combination of signs of the halves


def test_walk_replay_reaches_every_class():
    reachable = {"infinity+point", "general"}
    seen = collections.Counter()
    for x in WALK_SCALARS:
        for k in POINT_LOGS:
            got, classes = replay(x, k)
            assert got == x * k % N, (hex(x), k)
            assert set(classes) <= (reachable if k else {"table-infinity"}), (hex(x), k, classes)
            seen += classes
    assert set(seen) == reachable | {"table-infinity"}
    rng = random.Random(22)
    for _ in range(2000):
        x, k = rng.randrange(2**256), rng.randrange(1, N)
        got, classes = replay(x, k)
        assert got == x * k % N and set(classes) <= reachable
