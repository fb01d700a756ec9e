"""The scan under many view secrets on the host, no GPU: rangeproof.scan_keys_host (the literal K x rows loop over scan_host) on rec_test and
bin_test; the library's key recoding against a restatement; and a lane-for-lane replay of the shipped multi-key walk (csrc/rpscan_keys.hip.h) on
integers mod n, its table stage included.

The shipped form is a width-4 signed sliding window (wNAF) over each GLV half of a = a1 + a2 lambda, over the table P, 3P, 5P, 7P: per position,
from the highest down, one doubling, then +-m P for a digit +-m of a1 and +-m lambda P for a digit of a2.  Points are discrete logs (P = k G is
the integer k, infinity is 0).  Every addition is classified the way the complete law branches, with test_seal_scan_host's names:
    table-infinity   the table point is infinity (P is)         infinity+point   the accumulator is infinity
    doubling         the accumulator equals the table point     cancelling       the accumulator is the table point's negative
    general          none of these
Which can a walk reach?  Before the addition at position i the accumulator is u P with u = 2 (v >> (i + 1)) (+ the a1 digit of position i, for the
a2 addition), v the pair of halves as their wNAF prefixes; it meets a table entry t P (t = +-m or +-m lambda, m <= 7) only if u -+ t is zero or
a non-zero vector of the lattice of pairs that are 0 mod n, whose norm is at least n.  Zero: the prefix above position i is zero only before the
first addition (infinity+point), and a non-zero wNAF prefix times two never equals a single digit m <= 7 of the same half at the same position
unless the prefix is m / 2, which is not an integer for odd m; across halves (u in a1 only, t in a2 only) the difference is zero only for u = 0.
A lattice vector: prefixes are a / 2^i up to a digit, so for i >= 1 their norm, and that of the difference with an entry of norm <= 49, stays
below n (replay asserts it at every such step, as test_seal_scan_host does for the joint walk); at i = 0 the sum after the addition is a itself,
zero only for the scalar 0, which has no digit.  So for a point of prime order a walk reaches infinity+point and general, plus table-infinity for
P at infinity; the table stage reaches a doubling (2P, by the affine doubling, not an addition), then general additions (P + 2P, 3P + 2P, 5P + 2P)
or none for infinity.  test_walk_replay_reaches_every_class asserts exactly that over the scalars and points the GPU test runs."""
import collections
import ctypes as C
import json
import os
import random

import numpy as np

import pyoracle as O
from bulletproofspp_amd import capi, encoding
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from rp_backends import OracleBackend
from test_rangeproof import EXAMPLES
from test_seal_scan_host import POINT_LOGS, WALK_SCALARS

N, LAMBDA = O.N, O.LAMBDA
TAG = b"scan keys tag"
FOREIGN, OWNED, BAD_HINT, TAG_ONLY = RP.SCAN_FOREIGN, RP.SCAN_OWNED, RP.SCAN_BAD_HINT, RP.SCAN_TAG_ONLY


def _setups(oracle_lib):
    be = OracleBackend(oracle_lib)
    typed = RP.setup_from_schema(be, json.load(open(os.path.join(EXAMPLES, "rec_test", "schema.json"))))
    binary = BRP.setup_from_schema(be, json.load(open(os.path.join(EXAMPLES, "bin_test", "schema.json"))))
    return be, typed, binary


def test_scan_keys_host_orders_hits_and_ranks_row_verdicts(oracle_lib):
    ec = oracle_lib
    be, typed, binary = _setups(oracle_lib)
    for st in (typed, binary):
        rng = random.Random("scan keys host %d" % (st is typed))
        g, H0, B = RP._excess_bases(st)
        nr = len(st.rds)
        a, other = rng.randrange(1, N), rng.randrange(1, N)
        secrets = [a, other, a]                                              # two equal secrets: each is reported
        keys = [RP.excess_key33(ec.mul(s, B)) for s in (a, other)]
        # row b is sealed to a (even) or to other (odd); row 3 gets a bad hint, row 4 a flipped memo bit
        files, seals, openings = [], [], []
        for b in range(12):
            outs = [(rng.randrange(2**32), rng.randrange(N) if H0 is not None else 0) for _ in range(nr)]
            status, seal, blinds = RP.seal_host(be, st, keys[b & 1], rng.randrange(1, N), outs, TAG)
            assert status == RP.SEAL_OK
            coms = [ec.inner_product([(v % N, g), (bl, B)] + ([(ty, H0)] if H0 is not None else [])) for (v, ty), bl in zip(outs, blinds)]
            files.append(encoding.encode_commitments(coms)); seals.append(seal)
            openings.append([(v % N, ty, bl) for (v, ty), bl in zip(outs, blinds)])
        seals[3] = seals[3][:32] + b"\x02" + seals[3][33:]
        flipped = bytearray(seals[4]); flipped[34 + 64 + 31] ^= 1; seals[4] = bytes(flipped)
        row_status, hits, ntag = RP.scan_keys_host(be, st, secrets, files, seals, TAG)
        single = [[RP.scan_host(be, st, s, f, sl, TAG) for f, sl in zip(files, seals)] for s in secrets]
        # hits: every owned pair, by (row, key) ascending, with the opening of that row
        want_hits = [(k, i, single[k][i][1]) for i in range(12) for k in range(3) if single[k][i][0] == OWNED]
        assert hits == want_hits and [(i, k) for k, i, _ in hits] == sorted((i, k) for k, i, _ in hits)
        for i in range(12):
            if i in (3, 4):
                assert not [h for h in hits if h[1] == i]
            elif i & 1:
                assert [h for h in hits if h[1] == i] == [(1, i, openings[i])]
            else:
                assert [h for h in hits if h[1] == i] == [(0, i, openings[i]), (2, i, openings[i])]
        # row_status: BAD_HINT before OWNED before TAG_ONLY before FOREIGN
        assert row_status[3] == BAD_HINT and row_status[4] == TAG_ONLY
        assert all(row_status[i] == OWNED for i in range(12) if i not in (3, 4))
        assert single[0][4][0] == single[2][4][0] == TAG_ONLY
        assert ntag == sum(v == TAG_ONLY for col in single for v, _ in col) >= 2
        # a row that one key owns and another only tag-matches is OWNED; one that nobody's tag matches is FOREIGN
        foreign_only = RP.scan_keys_host(be, st, [other], files[:1], seals[:1], TAG)
        assert foreign_only[0][0] in (FOREIGN, TAG_ONLY) and foreign_only[1] == []
        assert RP.scan_keys_host(be, st, secrets, [], [], TAG) == ([], [], 0)


def wnaf4(m):
    """width-4 wNAF of m >= 0, digits from position 0 up"""
    out = []
    while m:
        d = 0
        if m & 1:
            d = m & 15
            if d > 8:
                d -= 16
            m -= d
        out.append(d)
        m >>= 1
    return out


def py_recode(x):
    """the recoding of csrc/rpscan_keys_plan.hpp restated: (digits of a1, digits of a2), signs folded in, both padded to the longer one"""
    a, b = O.decompose_eis(x % N)
    assert (a + b * LAMBDA - x) % N == 0
    d1, d2 = [-d if a < 0 else d for d in wnaf4(abs(a))], [-d if b < 0 else d for d in wnaf4(abs(b))]
    n = max(len(d1), len(d2))
    return d1 + [0] * (n - len(d1)), d2 + [0] * (n - len(d2))


def lib_recode(x):
    tl = capi.load_test_library()
    s, out = capi.int_to_limbs(x), np.full(36, 0xA5A5A5A5, dtype=np.uint32)
    assert tl.bppp_test_rp_scan_keys_recode(C.c_void_p(s.ctypes.data), C.c_void_p(out.ctypes.data)) == 0
    assert not out[34:].any()
    nbits = int(out[33])
    nib = lambda v: 0 if v == 0 else (2 * (v & 7) - 1) * (-1 if v & 8 else 1)
    by = [(int(out[i >> 2]) >> (8 * (i & 3))) & 0xFF for i in range(132)]
    assert nbits <= 132 and not any(by[nbits:])                              # nothing above the highest position
    assert all((v & 7) <= 4 and v != 8 for b in by for v in (b & 15, b >> 4))
    return [nib(b & 15) for b in by[:nbits]], [nib(b >> 4) for b in by[:nbits]]


def test_recoding_equals_the_restatement_and_is_a_wnaf():
    rng = random.Random(31)
    for x in WALK_SCALARS + [0, N - 2, 3] + [rng.randrange(2**256) for _ in range(64)]:
        d1, d2 = lib_recode(x)
        assert (d1, d2) == py_recode(x), hex(x)
        a = O.decompose_eis(x % N)
        for d, h in ((d1, a[0]), (d2, a[1])):
            assert sum(v << i for i, v in enumerate(d)) == h                 # the digits recompose to the signed half
            assert all(v == 0 or (v & 1 and abs(v) <= 7) for v in d)         # odd digits of magnitude at most 7
            nz = [i for i, v in enumerate(d) if v]
            assert all(j - i >= 4 for i, j in zip(nz, nz[1:]))               # no two non-zero digits within four places
        assert not d1 or d1[-1] or d2[-1]                                    # the highest position holds a digit
    assert lib_recode(N) == ([], []) and lib_recode(0) == ([], [])
    signs = {tuple(h < 0 for h in O.decompose_eis(x % N)) for x in WALK_SCALARS}
    assert len(signs) == 4                                                   # every combination of signs of the halves is folded into digits


def replay(x, k):
    """(x k mod n as the multi-key walk computes it, the classes of its additions) for P = k G: the table first, as scan_keys_table_lane makes
    it, then the walk of one key as scan_keys_mul_lane reads it"""
    classes = collections.Counter()

    def add(acc, t, where=""):
        cls = "table-infinity" if t == 0 else "infinity+point" if acc == 0 else "doubling" if acc == t else "cancelling" if (acc + t) % N == 0 else "general"
        classes[where + cls] += 1
        return (acc + t) % N
    tab = [0, 0, 0, 0]
    if k:                                                                    # the kernel makes no multiple of infinity: every entry stays zero
        two = 2 * k % N
        classes["table:doubling"] += 1
        tab[0] = k
        tab[1] = add(two, k, "table:")
        tab[2] = add(tab[1], two, "table:")
        tab[3] = add(tab[2], two, "table:")
    d1, d2 = lib_recode(x)
    a = O.decompose_eis(x % N)
    norm = lambda u, v: u * u - u * v + v * v
    assert 10 * norm(*a) < 39 * N
    acc, u = 0, [0, 0]                                                       # acc = (u[0] + u[1] lambda) k
    for i in range(len(d1) - 1, -1, -1):
        acc, u = 2 * acc % N, [2 * u[0], 2 * u[1]]
        for half, d in ((0, d1[i]), (1, d2[i])):
            if d:
                t = tab[(abs(d) - 1) // 2] * (LAMBDA if half else 1) % N
                t = (-t) % N if d < 0 else t
                for sign in (1, -1):                                         # neither u - t nor u + t is a lattice vector: no doubling, no cancelling
                    w = list(u); w[half] += sign * d
                    assert i == 0 or not any(u) or 0 < norm(*w) < N
                acc = add(acc, t)
                u[half] += d
        assert (u[0] + u[1] * LAMBDA) * k % N == acc
    return acc, classes


def test_walk_replay_reaches_every_class():
    reachable = {"infinity+point", "general", "table:doubling", "table:general"}
    seen = collections.Counter()
    for x in WALK_SCALARS:
        for k in POINT_LOGS:
            got, classes = replay(x, k)
            assert got == x * k % N, (hex(x), k)
            assert set(classes) <= (reachable if k else {"table-infinity"}), (hex(x), k, classes)
            if k:
                assert classes["table:general"] == 3 and classes["table:doubling"] == 1
            seen += classes
    assert set(seen) == reachable | {"table-infinity"}
    rng = random.Random(32)
    for _ in range(2000):
        x, k = rng.randrange(2**256), rng.randrange(1, N)
        got, classes = replay(x, k)
        assert got == x * k % N and set(classes) <= reachable
