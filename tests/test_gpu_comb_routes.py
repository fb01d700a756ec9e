"""Every route of the fixed-base comb (csrc/comb.hip.h), launched directly through the bppp_test_comb_* hooks of libbppp_hip_test.so and compared,
instance by instance and bit for bit, with a reference that shares nothing with the library: the basis is P_i = k_i G with k_i known to the test
(an arithmetic progression built with the C oracle's additions; k_1 = 0 is an infinity point, P_3 = P_2 a repeated one), so the result of an instance is
(sum_j s_j k_j mod n) G — Python integers and ONE oracle scalar multiplication.  Every instance of every launch is checked; a few instances per case
are also compared with the oracle's innerProduct over the points themselves, so that a slip in the bookkeeping of the k_i cannot cancel out.

Each test first asserts the route and the split the launcher reports (bppp_test_last_comb_msm), so a later change of the heuristics cannot move a case
onto another kernel unnoticed.  The expectations are comb_msm's arithmetic, restated in _plan below and pinned as literals in
test_the_plan_arithmetic_names_the_routes_the_cases_rely_on.

The scalars (_specials, _make_rows) sit where a comb breaks: the sign fold at n / 2, digits of magnitude D = 2^(c-1) and D - 1, values one either side of a
window boundary and of the carry into the next window (the `nw` early exit of k_comb_msm and its window-range split), rows of zeros, ones, the
argument's R zero pattern, a single non-zero last term, a sum that is 0 mod n, and random scalars over the WHOLE of [0, n).

The unmarked tests at the top are the CPU-only properties the GPU cases rely on."""
import ctypes
import functools
import random

import numpy as np
import pytest

import pyoracle as O

N = O.N
HALF = (N - 1) // 2
G = (O.GX, O.GY)
ANY, PAIRS, DENSE = 0, 1, 2
WAVE, PACKED8, PACKED16, ROWS, ROWS_PAIRS = 0, 1, 2, 3, 4          # bppp_test_comb_report.route
XYZZ = 160                                                           # bytes of one parked partial sum
ERR_ARG = -1
SENTINEL = 0xA5A5A5A5A5A5A5A5
K0 = 0x6A09E667F3BCC908B2FB1366EA957D3E3ADEC17512775099DA2F590B0667322A % N
KQ = 0x243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C89 % N
T_MAX = 4100


# ----------------------------------------------------------------------------- the format and the launcher's arithmetic, restated
def _windows(c):
    return -(-257 // c)


def _digits(s, c):
    """recode.hip.h as the comb reads it (all W windows c bits wide, all biased): (negated, folded value, signed digits)"""
    W, D = _windows(c), 1 << (c - 1)
    neg = s > N - s
    v = N - s if neg else s
    sp = v + sum(1 << (c * w + c - 1) for w in range(W))
    ds = [((sp >> (c * w)) & ((1 << c) - 1)) - D for w in range(W)]
    assert sp >> (c * W) == 0 and sum(d << (c * w) for w, d in enumerate(ds)) == v
    return neg, v, ds


def _nw(v, c):
    """k_comb_msm's early exit: windows a folded value v > 0 is walked through"""
    return -(-v.bit_length() // c) + 1


def _plan(ninst, nterms, hint, scratch, rows_waves=0, rows_table=False):
    """comb_msm_launch's choice (csrc/comb.hip.h); rows_table: the table is at least BPPP_COMB_ROWS_MIN_MB large"""
    if nterms <= 48 and ninst >= 512:
        return dict(route=PACKED8 if nterms <= 24 else PACKED16)
    if hint != ANY and scratch and ninst >= 512 and nterms >= 256 and rows_table:
        pairs = hint == PAIRS and ninst % 2 == 0
        ngroups = ((ninst // 2 if pairs else ninst) + 63) // 64
        gtot = 2 * ngroups if pairs else ngroups
        chunks = max(1, min(nterms // 4, (min(rows_waves or 16384, 16384) + gtot - 1) // gtot))
        while chunks > 1 and ninst * chunks * XYZZ > scratch:
            chunks -= 1
        clen = -(-nterms // chunks)
        chunks = -(-nterms // clen)
        if ninst * chunks * XYZZ <= scratch:
            lanes = 4
            while lanes < 64 and lanes * 12 < chunks:
                lanes *= 2
            return dict(route=ROWS_PAIRS if pairs else ROWS, chunks=chunks, clen=clen, join_lanes=lanes)
    tparts = wsplit = 1
    groups = (nterms + 63) // 64
    target = 8192 if groups >= 32 else 1024
    if scratch and ninst < target and groups > 1:
        tparts = min(groups, 64, -(-target // ninst))
        while tparts > 1 and ninst * tparts * XYZZ > scratch:
            tparts -= 1
        if tparts == groups:
            wsplit = min(64 // tparts, 4, 1024 // max(1, ninst * tparts))
            while wsplit > 1 and ninst * tparts * wsplit * XYZZ > scratch:
                wsplit -= 1
            wsplit = max(wsplit, 1)
    return dict(route=WAVE, parts=tparts * wsplit, tparts=tparts, wsplit=wsplit, heavy_first=int(hint == PAIRS and ninst % 2 == 0))


def _full_scratch(ninst, nterms):
    """room for either route: 64 partial sums per instance, and the rows route's nterms / 4"""
    return ninst * max(64, nterms // 4 + 1) * XYZZ


# ----------------------------------------------------------------------------- scalars
def _specials(c, w0s=()):
    W, D = _windows(c), 1 << (c - 1)
    vals = [0, 1, N - 1, HALF, HALF + 1, HALF - 1, HALF + 2, 2**255 % N, (2**255 - 1) % N]
    for k in sorted({1, 2, W // 2, W - 2, W - 1, *w0s}):
        for x in (2**(c * k - 1) - 1, 2**(c * k - 1), 2**(c * k - 1) + 1, 2**(c * k) - 1, 2**(c * k)):
            if 0 < x < N:
                vals += [x, N - x]
    wtop = max(w for w in range(W) if (D - 1) << (c * w) <= HALF)
    for w in (0, W // 2, wtop):                                     # a digit of exactly D - 1 in the bottom, a middle and the top window
        vals += [(D - 1) << (c * w), N - ((D - 1) << (c * w))]
    return vals


def _logs(T):
    ks = [(K0 + i * KQ) % N for i in range(T)]
    if T > 1:
        ks[1] = 0
    if T > 3:
        ks[3] = ks[2]
    return ks


@functools.lru_cache(maxsize=None)
def _make_rows(ninst, nterms, c, seed, w0s=(), pairs=False):
    """(rows, share that folds among the random draws still in the rows): the shared generator.  Random over [0, n) everywhere, then the special
    values at the hot positions (first and last term, the last lane's term, either side of the 64-term group boundaries and of short chunk ends; with
    fewer than 16 instances also every fifth position, and in rows of at most 8 terms every other position only, so that random draws remain) and,
    with 16 or more instances, the pattern rows: 0 all zero, 1 all one, 2 zero on even indices, 3 zero where (i >> 1) & 1 == 0, 4 only the last term,
    5 (6 with pairs) a sum that is 0 mod n.  pairs: every odd row also carries the R zero pattern; the even rows are dense except for the pattern
    rows 0, 2 and 4 of the 514- and 515-instance cases, which keep their zeros."""
    rnd = random.Random(f"{ninst} {nterms} {c} {seed}")
    ks = _logs(T_MAX)
    rows = [[rnd.randrange(N) for _ in range(nterms)] for _ in range(ninst)]
    drawn = [list(r) for r in rows]
    sp = _specials(c, w0s)
    hot = sorted(p for p in {0, nterms - 1, nterms - 2, 3, 4, 5, 7, 8, 15, 16, 62, 63, 64, 65, 127, 128, (nterms - 1) // 64 * 64, (nterms - 1) // 64 * 64 - 1} if 0 <= p < nterms)
    j = seed
    first = 0
    if ninst >= 16:
        first = 7
        rows[0] = [0] * nterms
        rows[1] = [1] * nterms
        rows[2] = [s if i & 1 else 0 for i, s in enumerate(rows[2])]
        rows[3] = [s if (i >> 1) & 1 else 0 for i, s in enumerate(rows[3])]
        rows[4] = [0] * (nterms - 1) + [rows[4][-1] or 1]
    for r in range(first, ninst):
        where = hot + list(range(r % 5, nterms, 5)) if ninst < 16 else [hot[(r + 3 * t) % len(hot)] for t in range(4)] + [(7 * r) % nterms]
        if ninst < 16 and nterms <= 8:
            where = [p for p in range(nterms) if (p + r) & 1]
        for p in where:
            rows[r][p] = sp[j % len(sp)]
            j += 1
    if pairs:
        for r in range(1, ninst, 2):
            rows[r] = [s if (i >> 1) & 1 else 0 for i, s in enumerate(rows[r])]
    if ninst >= 16:
        z = 6 if pairs else 5
        jz = max(i for i in range(nterms) if ks[i])
        rest = sum(s * k for i, (s, k) in enumerate(zip(rows[z], ks)) if i != jz) % N
        rows[z][jz] = (-rest * pow(ks[jz], -1, N)) % N
    left = [s for r, d in zip(rows, drawn) for s, s0 in zip(r, d) if s == s0]
    return rows, (sum(1 for s in left if s > N - s) / len(left) if left else None)


def _pt_bytes(p):
    return bytes(64) if p is None else p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")


def _times_g(ec, es):
    """e G for every e, as result bytes: one oracle scalar multiplication each, on a few threads (the C oracle holds no state and ctypes
    releases the interpreter lock during a call)"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(lambda e: _pt_bytes(ec.mul(e, G)), es, chunksize=64))


def _rows_array(rows):
    return np.frombuffer(b"".join(s.to_bytes(32, "little") for r in rows for s in r), dtype=np.uint64).copy()


# every (ninst, nterms, c, seed, w0s, pairs) the GPU cases generate: the fold share is asserted for each of them on the CPU
W0_C5 = (13, 26, 39)                                                # c = 5: W = 52, four window ranges of 13
CASES_ROWS = [(515, n, 5, 1, (), False) for n in (256, 259, 400, 780, 1540)]
CASES_PAIRS = [(514, 259, 5, 2, (), True), (515, 259, 5, 2, (), True)]
CASES_FEW = [(1, 775, 5, 3, W0_C5, False), (2, 775, 5, 3, W0_C5, False), (5, 775, 5, 3, W0_C5, False), (3, 4099, 5, 3, W0_C5, False), (6, 775, 5, 3, W0_C5, True),
             (7, 775, 5, 3, W0_C5, True)]
CASES_PACKED = [(515, n, 5, 4, (), False) for n in (1, 24, 25, 48)] + [(511, 48, 5, 4, (), False)]
GROUP_SHAPES = [(261, 512, 1), (261, 512, 5), (5, 3, 3), (1, 1, 1), (0, 8, 2)]
CASES_GROUPS = [(ninst, 1 + l0 + n0, 5, 5, (), False) for ninst in (5, 64, 70) for l0, n0, _ in GROUP_SHAPES]
LANES_SEED = 10                                                     # (the first seed with which the few draws of the one-instance cases fold too)
CASES_LANES = [(ninst, n, 5, LANES_SEED, (), False) for n in (1, 3, 5) for ninst in (1, 63, 65, 1000)]
WIDE = {16: 8, 18: 4, 4: 80}                                        # window bits -> points of the table
CASES_WIDE = [(ninst, n, c, 7, (), False) for c, T in WIDE.items() for ninst, n in ((65, min(3, T)), (70, T), (515, 4), (515, min(8, T)))]
ALL_CASES = sorted(set(CASES_ROWS + CASES_PAIRS + CASES_FEW + CASES_PACKED + CASES_GROUPS + CASES_LANES + CASES_WIDE))


# ----------------------------------------------------------------------------- CPU-only: what the GPU cases rely on
def test_at_least_a_third_of_every_cases_random_scalars_fold():
    """random scalars are drawn over all of [0, n), so about half exceed n / 2 and take the negating fold (a draw below 2^255 almost never would)"""
    for case in ALL_CASES:
        rows, folds = _make_rows(*case)
        assert folds is not None and folds >= 1 / 3, (case, folds)
        assert all(0 <= s < N for r in rows for s in r)
    assert sum(s > N - s for s in _specials(5)) >= len(_specials(5)) // 3


@pytest.mark.parametrize("c", [4, 5, 13, 16, 18])
def test_the_boundary_values_have_the_digits_they_are_named_for(c):
    W, D = _windows(c), 1 << (c - 1)
    assert c * W >= 257 and c * (W - 1) < 257
    for k in {1, 2, W // 2, W - 2, W - 1} | (set(W0_C5) if c == 5 else set()):
        if 2**(c * k - 1) > HALF:
            continue
        neg, v, ds = _digits(2**(c * k - 1), c)                     # digit -D in window k - 1 and the carry 1 in window k: the last window `nw` keeps
        assert not neg and ds[k - 1] == -D and ds[k] == 1 and not any(ds[k + 1:]) and not any(ds[:k - 1]) and _nw(v, c) == k + 1
        neg, v, ds = _digits(2**(c * k - 1) - 1, c)                 # one below: D - 1 alone in window 0, or -1 at the bottom and the same -D and carry
        assert (ds[0] == D - 1 and not any(ds[1:])) if k == 1 else (ds[0] == -1 and ds[k - 1] == -D and ds[k] == 1 and not any(ds[1:k - 1]))
        assert _nw(v, c) == k + 1
        neg, v, ds = _digits(N - 2**(c * k - 1), c)                 # the same magnitudes through the fold
        assert neg and ds[k - 1] == -D and ds[k] == 1
        if 2**(c * k) <= HALF:
            neg, v, ds = _digits(2**(c * k), c)                     # one bit into window k: a wavefront whose range starts at w0 = k has work, the one before has none
            assert ds[k] == 1 and not any(ds[:k]) and _nw(v, c) == k + 2
            neg, v, ds = _digits(2**(c * k) - 1, c)                 # digit -1 at the bottom, zeros, and the carry 1 into window k
            assert ds[0] == -1 and not any(ds[1:k]) and ds[k] == 1 and _nw(v, c) == k + 1
    wtop = max(w for w in range(W) if (D - 1) << (c * w) <= HALF)
    for w in (0, W // 2, wtop):
        neg, v, ds = _digits((D - 1) << (c * w), c)
        assert not neg and ds[w] == D - 1 and sum(1 for d in ds if d) == 1
    neg, v, ds = _digits(HALF + 1, c)                               # (n + 1) / 2 folds onto (n - 1) / 2, the largest folded value
    assert neg and v == HALF and _digits(HALF, c)[2] == ds
    # no value walks past its `nw` windows: every digit from there on is zero (what the early exit of k_comb_msm relies on)
    for s in _specials(c, W0_C5 if c == 5 else ()):
        neg, v, ds = _digits(s, c)
        assert v == 0 or not any(ds[_nw(v, c):]), hex(s)
    assert {abs(d) for s in _specials(c) for d in _digits(s, c)[2]} >= {D, D - 1, 1}


def test_the_plan_arithmetic_names_the_routes_the_cases_rely_on():
    big = 1 << 40
    rows = lambda ninst, nterms, hint, scratch, waves=0: _plan(ninst, nterms, hint, scratch, waves, True)
    # a. 515 dense rows: 9 groups of 64; nterms / 4 chunks at most, evened out by clen = ceil(nterms / chunks).  (256 terms: 64 chunks of 4; 259: clen 5, so 52)
    assert rows(515, 259, DENSE, big) == dict(route=ROWS, chunks=52, clen=5, join_lanes=8)
    assert rows(515, 256, DENSE, big) == dict(route=ROWS, chunks=64, clen=4, join_lanes=8)
    assert rows(515, 259, DENSE, big, 9) == dict(route=ROWS, chunks=1, clen=259, join_lanes=4) and rows(515, 256, DENSE, big, 9)["chunks"] == 1
    assert [rows(515, n, DENSE, big)["chunks"] for n in (400, 780, 1540)] == [100, 195, 385]          # > 96, > 192, > 384
    assert [rows(515, n, DENSE, big)["join_lanes"] for n in (400, 780, 1540)] == [16, 32, 64]
    assert rows(515, 259, DENSE, 515 * 20 * XYZZ) == dict(route=ROWS, chunks=20, clen=13, join_lanes=4)     # the scratch holds 20 partial sums per row
    assert rows(515, 259, DENSE, XYZZ) == dict(route=WAVE, parts=1, tparts=1, wsplit=1, heavy_first=0)      # not even one: k_comb_msm, unsplit
    # b. pairs only for an even count
    assert rows(514, 259, PAIRS, big)["route"] == ROWS_PAIRS and rows(515, 259, PAIRS, big)["route"] == ROWS
    assert _plan(514, 259, PAIRS, big)["route"] == WAVE             # a small table on a default context: not the rows route
    # c. few instances: 13 groups of 64 terms x 4 window ranges; 65 groups: 64 term parts and no window split
    for ninst in (1, 2, 5):
        assert _plan(ninst, 775, ANY, big) == dict(route=WAVE, parts=52, tparts=13, wsplit=4, heavy_first=0)
        assert _plan(ninst, 775, ANY, 0)["parts"] == 1 and _plan(ninst, 775, ANY, 2 * ninst * XYZZ) == dict(route=WAVE, parts=2, tparts=2, wsplit=1, heavy_first=0)
    assert _plan(3, 4099, ANY, big) == dict(route=WAVE, parts=64, tparts=64, wsplit=1, heavy_first=0)
    assert _plan(6, 775, PAIRS, big) == dict(route=WAVE, parts=52, tparts=13, wsplit=4, heavy_first=1)
    assert _plan(7, 775, PAIRS, big) == dict(route=WAVE, parts=52, tparts=13, wsplit=4, heavy_first=0)
    assert -(-_windows(5) // 4) == 13 and W0_C5 == (13, 26, 39)
    # d. packed from 512 instances of at most 48 terms on
    assert [_plan(515, n, ANY, 0)["route"] for n in (1, 24, 25, 48)] == [PACKED8, PACKED8, PACKED16, PACKED16]
    assert _plan(511, 48, ANY, big) == dict(route=WAVE, parts=1, tparts=1, wsplit=1, heavy_first=0)
    # g. 70 instances of 80 terms at c = 4: two term parts x four ranges of 17 of the 65 windows
    assert _plan(70, 80, ANY, big) == dict(route=WAVE, parts=8, tparts=2, wsplit=4, heavy_first=0) and _windows(4) == 65
    assert _plan(70, 8, ANY, big)["parts"] == 1
    for ninst, nterms in ((515, 1540), (514, 259), (5, 775), (3, 4099), (70, 80)):
        assert _full_scratch(ninst, nterms) >= ninst * max(64, nterms // 4) * XYZZ


# ----------------------------------------------------------------------------- the GPU side
class Table:
    """a comb table of the first T basis points on context g, and the three launchers on it"""

    def __init__(self, g, pts_arr, T, c):
        from bulletproofspp_amd.capi import load_test_library
        self.g, self.tl, self.T, self.c, self.h = g, load_test_library(), T, c, None
        d = g.to_device(np.ascontiguousarray(pts_arr[:T]))
        h = ctypes.c_void_p()
        try:
            rc = self.tl.bppp_test_comb_create(g.h, d, T, c, ctypes.byref(h))
        finally:
            g.free(d)
        assert rc == 0, g.lib.bppp_last_error(g.h)
        self.h = h

    def close(self):
        if self.h:
            self.tl.bppp_test_comb_destroy(self.h)
            self.h = None

    def _run(self, rows, words, call):
        d = self.g.to_device(_rows_array(rows))
        out = np.full(words, SENTINEL, dtype=np.uint64)
        try:
            rc = call(d, out.ctypes.data)
        finally:
            self.g.free(d)
        return rc, out

    def msm(self, rows, hint=ANY, scratch=0, nterms=None):
        from bulletproofspp_amd.capi import TestCombReport
        nterms = len(rows[0]) if nterms is None else nterms
        rc, out = self._run(rows, len(rows) * 8, lambda d, o: self.tl.bppp_test_comb_msm(self.h, d, len(rows), nterms, hint, scratch, o))
        assert rc == 0, (rc, self.g.lib.bppp_last_error(self.g.h))
        rep = TestCombReport()
        assert self.tl.bppp_test_last_comb_msm(self.g.h, ctypes.byref(rep)) == 0
        rep = {n: getattr(rep, n) for n, _ in TestCombReport._fields_}
        if rep["route"] == WAVE:
            rep = {n: rep[n] for n in ("route", "parts", "tparts", "wsplit", "heavy_first")}
        elif rep["route"] in (ROWS, ROWS_PAIRS):
            rep = {n: rep[n] for n in ("route", "chunks", "clen", "join_lanes")}
        else:
            rep = {"route": rep["route"]}
        return out, rep

    def groups(self, rows, l0, n0, L, stride):
        return self._run(rows, len(rows) * stride * 8, lambda d, o: self.tl.bppp_test_comb_groups(self.h, d, len(rows), l0, n0, L, stride, o))

    def lanes(self, rows, nterms=None):
        nterms = len(rows[0]) if nterms is None else nterms
        return self._run(rows, len(rows) * 8, lambda d, o: self.tl.bppp_test_comb_lanes(self.h, d, nterms, len(rows), o))


@pytest.fixture(scope="module")
def basis(oracle_lib):
    """(k_i, P_i = k_i G as points, as an array): P_0 = K0 G and steps of KQ G by oracle additions; k_1 = 0, P_3 = P_2"""
    ks = _logs(T_MAX)
    step, p, pts = oracle_lib.mul(KQ, G), oracle_lib.mul(K0, G), []
    for _ in range(T_MAX):
        pts.append(p)
        p = oracle_lib.add(p, step)
    pts[1], pts[3] = None, pts[2]
    for i in (0, 1, 2, 3, 4, 777, T_MAX - 1):
        assert pts[i] == oracle_lib.mul(ks[i], G)
    from bulletproofspp_amd.capi import points_to_array
    return ks, pts, points_to_array(pts)


@pytest.fixture(scope="module")
def want(oracle_lib, basis):
    """want(case) -> (rows, the expected 64 bytes of every instance), computed once per case and shared; the instances named in `cross` are also
    compared with the oracle's innerProduct over the points"""
    ks, pts, _ = basis
    cache = {}

    def get(case, cross=()):
        if case not in cache:
            rows, _ = _make_rows(*case)
            exp = _times_g(oracle_lib, [sum(s * k for s, k in zip(r, ks)) % N for r in rows])
            for b in cross:
                b %= len(rows)
                assert _pt_bytes(oracle_lib.inner_product(list(zip(rows[b], pts)))) == exp[b], (case, b)
            if len(rows) >= 16:
                assert exp[0] == bytes(64) and exp[6 if case[5] else 5] == bytes(64) and exp[1] != bytes(64)
            cache[case] = (rows, exp)
        return cache[case]
    return get


def _same(out, exp, what):
    raw = out.tobytes()
    assert len(raw) == 64 * len(exp)
    if raw != b"".join(exp):
        bad = [i for i, w in enumerate(exp) if raw[64 * i:64 * i + 64] != w]
        pytest.fail(f"{what}: {len(bad)} of {len(exp)} instances differ from the reference, first {bad[:10]}")


def _context(env):
    """a context of its own, made under the tuning variables `env` (read once, at creation)"""
    import bulletproofspp_amd as b
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return b.Bppp(0)


@pytest.fixture(scope="module")
def rows_table(basis):
    """c = 5 over 1600 points on a context where every table qualifies for the rows route"""
    g = _context({"BPPP_COMB_ROWS_MIN_MB": "0", "BPPP_COMB_ROWS_WAVES": "0"})
    t = Table(g, basis[2], 1600, 5)
    yield t
    t.close()
    g.close()


@pytest.fixture(scope="module")
def table5(gpu, basis):
    """c = 5 over all 4100 points on the default context (218 MB: below the rows route's table size)"""
    t = Table(gpu, basis[2], T_MAX, 5)
    yield t
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nterms,chunks,lanes", [(256, 64, 8), (259, 52, 8), (400, 100, 16), (780, 195, 32), (1540, 385, 64)])
def test_rows_dense_every_join_width(rows_table, want, nterms, chunks, lanes):
    """a. k_comb_msm_rows + k_comb_join_rows<8 .. 64>: 515 instances (8 groups of 64 and one of 3) over a prefix of a 1600-point table"""
    case = (515, nterms, 5, 1, (), False)
    rows, exp = want(case, cross=(7, 514) if nterms <= 800 else (514,))
    scratch = _full_scratch(515, nterms)
    out, rep = rows_table.msm(rows, DENSE, scratch)
    assert rep == dict(route=ROWS, chunks=chunks, clen=-(-nterms // chunks), join_lanes=lanes) == _plan(515, nterms, DENSE, scratch, 0, True)
    _same(out, exp, f"rows, {nterms} terms")


@pytest.mark.gpu
def test_rows_dense_one_chunk_and_the_four_lane_join(basis, want):
    """a. BPPP_COMB_ROWS_WAVES=9: one wavefront per group of 64 rows, a single chunk of the whole row, k_comb_join_rows<4>"""
    g = _context({"BPPP_COMB_ROWS_MIN_MB": "0", "BPPP_COMB_ROWS_WAVES": "9"})
    t = Table(g, basis[2], 300, 5)
    try:
        for nterms in (256, 259):
            rows, exp = want((515, nterms, 5, 1, (), False))
            out, rep = t.msm(rows, DENSE, _full_scratch(515, nterms))
            assert rep == dict(route=ROWS, chunks=1, clen=nterms, join_lanes=4) == _plan(515, nterms, DENSE, 1 << 40, 9, True)
            _same(out, exp, f"rows in one chunk, {nterms} terms")
    finally:
        t.close()
        g.close()


@pytest.mark.gpu
def test_rows_dense_under_a_short_scratch(rows_table, want):
    """a. a scratch of 20 partial sums per row walks `chunks` down from 64 (20 chunks of 13 terms, the last of 12); one that does not hold a single
    partial sum per row falls through to k_comb_msm, one wavefront per instance"""
    rows, exp = want((515, 259, 5, 1, (), False))
    out, rep = rows_table.msm(rows, DENSE, 515 * 20 * XYZZ)
    assert rep == dict(route=ROWS, chunks=20, clen=13, join_lanes=4) == _plan(515, 259, DENSE, 515 * 20 * XYZZ, 0, True)
    _same(out, exp, "rows, 20 chunks")
    out, rep = rows_table.msm(rows, DENSE, XYZZ)
    assert rep == dict(route=WAVE, parts=1, tparts=1, wsplit=1, heavy_first=0) == _plan(515, 259, DENSE, XYZZ, 0, True)
    _same(out, exp, "rows hint, no room: k_comb_msm")


@pytest.mark.gpu
@pytest.mark.parametrize("ninst,route", [(514, ROWS_PAIRS), (515, ROWS)])
def test_rows_pairs(rows_table, want, ninst, route):
    """b. 257 pairs (four groups of 64 pairs and one of a single pair), odd rows with the R zero pattern; an odd count runs without the pairing"""
    rows, exp = want((ninst, 259, 5, 2, (), True), cross=(8, 9))
    out, rep = rows_table.msm(rows, PAIRS, _full_scratch(ninst, 259))
    assert rep == dict(route=route, chunks=52, clen=5, join_lanes=8) == _plan(ninst, 259, PAIRS, 1 << 40, 0, True)
    _same(out, exp, f"rows with the pairs hint, {ninst} instances")


@pytest.mark.gpu
@pytest.mark.parametrize("ninst,nterms,hint,full", [(1, 775, ANY, (13, 4, 0)), (2, 775, ANY, (13, 4, 0)), (5, 775, ANY, (13, 4, 0)), (3, 4099, ANY, (64, 1, 0)),
                                                    (6, 775, PAIRS, (13, 4, 1)), (7, 775, PAIRS, (13, 4, 0))])
def test_few_instances_split_over_term_parts_and_window_ranges(table5, want, ninst, nterms, hint, full):
    """c. k_comb_msm + k_comb_join below 64 instances: term parts x window ranges with room for them, two term parts with room for two, one wavefront
    per instance without scratch; the PAIRS hint dispatches heavy first for an even count.  The boundary values sit at every range's first window."""
    rows, exp = want((ninst, nterms, 5, 3, W0_C5, hint == PAIRS), cross=(0, ninst - 1) if nterms < 800 else (1,))
    tparts, wsplit, hf = full
    for scratch, split in ((_full_scratch(ninst, nterms), dict(parts=tparts * wsplit, tparts=tparts, wsplit=wsplit)), (0, dict(parts=1, tparts=1, wsplit=1)),
                           (2 * ninst * XYZZ, dict(parts=2, tparts=2, wsplit=1))):
        out, rep = table5.msm(rows, hint, scratch)
        assert rep == dict(route=WAVE, heavy_first=hf, **split) == _plan(ninst, nterms, hint, scratch)
        _same(out, exp, f"{ninst} instances of {nterms} terms, scratch {scratch}")


@pytest.mark.gpu
@pytest.mark.parametrize("ninst,nterms,route", [(515, 1, PACKED8), (515, 24, PACKED8), (515, 25, PACKED16), (515, 48, PACKED16), (511, 48, WAVE)])
def test_packed_instances(table5, want, ninst, nterms, route):
    """d. k_comb_msm_packed<8 | 16>: 515 instances (a last wavefront of 3), terms at both ends of either width; 511 stay on k_comb_msm"""
    rows, exp = want((ninst, nterms, 5, 4, (), False), cross=(6, 7, ninst - 1))
    out, rep = table5.msm(rows, ANY, _full_scratch(ninst, nterms))
    assert rep == (dict(route=route) if route != WAVE else dict(route=WAVE, parts=1, tparts=1, wsplit=1, heavy_first=0)) == _plan(ninst, nterms, ANY, 1 << 40)
    _same(out, exp, f"packed, {ninst} x {nterms}")


@pytest.mark.gpu
@pytest.mark.parametrize("l0,n0,L", GROUP_SHAPES)
@pytest.mark.parametrize("ninst", [5, 64, 70])
def test_comb_groups(table5, basis, oracle_lib, ninst, l0, n0, L):
    """e. k_comb_msm_groups: sums of 2^L consecutive points of the lin part and of the norm part, short last groups, a group longer than its part;
    slot 0 and the slots past the groups keep the sentinel"""
    ks, pts, _ = basis
    nterms = 1 + l0 + n0
    rows, _ = _make_rows(ninst, nterms, 5, 5)
    l0r, n0r = -(-l0 // (1 << L)), -(-n0 // (1 << L))
    stride = 1 + l0r + n0r + 3
    rc, out = table5.groups(rows, l0, n0, L, stride)
    assert rc == 0
    ranges = [(1 + (q << L), min(1 + l0, 1 + ((q + 1) << L))) for q in range(l0r)] + [(1 + l0 + (q << L), min(nterms, 1 + l0 + ((q + 1) << L))) for q in range(n0r)]
    assert all(a < b for a, b in ranges) and sorted(i for a, b in ranges for i in range(a, b)) == list(range(1, nterms))
    ec = oracle_lib
    sent = np.full(8, SENTINEL, dtype=np.uint64).tobytes()
    sums = iter(_times_g(ec, [sum(r[i] * ks[i] for i in range(a, b)) % N for r in rows for a, b in ranges]))
    exp = []
    for r in rows:
        exp += [sent] + [next(sums) for _ in ranges] + [sent] * 3
    a, b = ranges[-1]
    assert exp[(ninst - 1) * stride + len(ranges)] == _pt_bytes(ec.inner_product([(rows[-1][i], pts[i]) for i in range(a, b)]))
    _same(out, exp, f"groups of 2^{L}, l0 {l0}, n0 {n0}, {ninst} instances")


@pytest.mark.gpu
def test_comb_groups_refusals(table5):
    """e. what comb_groups refuses comes back as BPPP_ERR_ARG and nothing is launched: the output keeps its sentinel"""
    rows = [[1] * 9 for _ in range(5)]
    for l0, n0, L, stride in ((T_MAX, 0, 1, 1 << 13), (T_MAX - 9, 9, 1, 1 << 13), (4, 4, 0, 16), (4, 4, 21, 16), (4, 4, 1, 4), (5, 3, 3, 2)):
        rc, out = table5.groups(rows, l0, n0, L, stride)
        assert rc == ERR_ARG and (out == SENTINEL).all(), (l0, n0, L, stride)
    rc, out = table5.groups(rows, 4, 4, 1, 5)                        # the shortest stride that holds 1 + 2 + 2 slots
    assert rc == 0 and (out.reshape(5, 5, 8)[:, 0] == SENTINEL).all() and not (out.reshape(5, 5, 8)[:, 1:] == SENTINEL).any()
    rc, out = table5.lanes(rows, nterms=T_MAX + 1)
    assert rc == ERR_ARG and (out == SENTINEL).all()
    d = table5.g.to_device(_rows_array(rows))
    try:
        o = np.full(5 * 8, SENTINEL, dtype=np.uint64)
        assert table5.tl.bppp_test_comb_msm(table5.h, d, 5, T_MAX + 1, ANY, 0, o.ctypes.data) == ERR_ARG and (o == SENTINEL).all()
    finally:
        table5.g.free(d)


@pytest.mark.gpu
@pytest.mark.parametrize("nterms", [1, 3, 5])
@pytest.mark.parametrize("ninst", [1, 63, 65, 1000])
def test_comb_lanes(table5, want, ninst, nterms):
    """f. k_comb_lanes: one lane per instance over the first 1, 3, 5 points (the second is infinity, the fourth repeats the third)"""
    rows, exp = want((ninst, nterms, 5, LANES_SEED, (), False), cross=(ninst - 1,))
    rc, out = table5.lanes(rows)
    assert rc == 0
    _same(out, exp, f"lanes, {ninst} x {nterms}")


@pytest.mark.gpu
@pytest.mark.parametrize("c", sorted(WIDE))
def test_the_widest_and_the_narrowest_windows(gpu, basis, want, c):
    """g. c = 16 (17 windows x 32768 multiples, 285 MB over 8 points) and c = 18 (15 x 131072, 503 MB over 4) — index arithmetic (w T D + mag - 1) with
    digits of magnitude exactly D and D - 1 in the bottom, a middle and the top window — and c = 4, 65 windows, whose bias reaches into the ninth limb:
    through comb_lanes, k_comb_msm at 70 instances and k_comb_msm_packed at 515"""
    T = WIDE[c]
    t = Table(gpu, basis[2], T, c)
    try:
        rows, exp = want((65, min(3, T), c, 7, (), False), cross=(64,))
        rc, out = t.lanes(rows)
        assert rc == 0
        _same(out, exp, f"lanes, c = {c}")
        rows, exp = want((70, T, c, 7, (), False), cross=(8, 69))
        out, rep = t.msm(rows, ANY, _full_scratch(70, T), nterms=0)          # 0: all T points of the table
        assert rep == dict(route=WAVE, heavy_first=0, **(dict(parts=8, tparts=2, wsplit=4) if c == 4 else dict(parts=1, tparts=1, wsplit=1))) == _plan(70, T, ANY, 1 << 40)
        _same(out, exp, f"70 instances, c = {c}")
        for nterms in sorted({4, min(8, T)}):
            rows, exp = want((515, nterms, c, 7, (), False), cross=(9,))
            out, rep = t.msm(rows, ANY, 0)
            assert rep == dict(route=PACKED8)
            _same(out, exp, f"packed, {nterms} terms, c = {c}")
    finally:
        t.close()
