"""The ranged scatter that reads a chunk's digits once (k_scatter_one_read; csrc/msm.hip, make_plan's MsmPlan::one_read): one workgroup per
(window, chunk) keeps its digits in registers and places bucket range 0, 1, ... from them, where k_scatter_ranges runs one workgroup per
(window, range, chunk) and reads the chunk again for every range.  The plan takes the form when no chunk is longer than the SCATTER_AHEAD =
4 steps of 1024 lanes x 8 digits a lane holds (32768 digits) and its 16 x CH workgroups fill their rounds on the CUs (_reads_once); else it
keeps k_scatter_ranges.

Every result is compared with the CPU oracle and, byte for byte, with the same call on a context created with BPPP_SCATTER_ONE_READ=0 (the
environment is read once per context); bppp_test_last_scatter_one_read says which kernel ran.  The hooks do not expose the sorted entries,
so the group element is the check of the positions too.

The oracle takes 170 us per term, so it is given an equal sum of 256 terms: the n points are 256 hashed points repeated, point i = base
point i mod 256, hence sum s_i P_i = sum_k (sum_{i = k mod 256} s_i mod N) B_k, and the inner sums are integer additions done here.

Sizes, from make_plan on 256 CUs (32 per XCD): with 16-bit windows CH = min(32, ceil(n / 32768)) chunks of ceil(n / CH) digits rounded up
to 8.  Without window_bits the plan takes 16-bit windows, and so the ranged scatter, from 200 000 terms on: 7 chunks, 112 workgroups, under
one round, k_scatter_ranges.  15 x 2^15 + 1 terms are the fewest with 16 chunks, a whole round, and so the fewest that read once: no
multiple of 8, the last chunk partial (30 601 of 30 728 digits).  17 x 2^15 have 272 workgroups, 16 of them in a second round, and keep
k_scatter_ranges.  2^20 has 32 chunks of exactly four steps; 2^20 + 1 has chunks of 32 776 digits, a fifth step for one lane, and takes
k_scatter_ranges.  With window_bits = 16 and 16 forced chunks (BPPP_HIST_CH=16) the form runs at any size: one term (15 empty chunks), 2^19
(exactly four steps) and 2^19 + 1 (the fallback again), and the scalar patterns at 70 001 terms."""
import ctypes
import os
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd.capi import points_to_array, scalars_to_array

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)
NBASE = 256
# (BPPP_SCATTER_ONE_READ, BPPP_HIST_CH): the default, the comparison (k_scatter_ranges), and both with 16 forced chunks (one round of 256 CUs)
CONFIGS = [("1", None), ("0", None), ("1", "16"), ("0", "16")]
FORCED = "16"
STEP, AHEAD, XCD_CUS, WINDOWS = 1024 * 8, 4, 32, 16


def _chunks(n, hist_ch):
    """make_plan's chunk count of the ranged scatter at 16-bit windows, and the steps per lane of its chunks"""
    ch = int(hist_ch) if hist_ch else min(XCD_CUS, max(1, -(-n // 65536), -(-(XCD_CUS * n) // (1 << 20))))
    per = (-(-n // ch) + 7) & ~7
    return ch, per, -(-per // STEP)


def _reads_once(n, hist_ch):
    """make_plan's rule for k_scatter_one_read: at most four steps per lane, and the 16 x CH workgroups (one per CU) are at least one whole
    round with no last round that fewer than a quarter of the CUs take part in"""
    ch, _, steps = _chunks(n, hist_ch)
    wgs, cus = WINDOWS * ch, 8 * XCD_CUS
    return steps <= AHEAD and wgs >= cus and not 0 < wgs % cus < cus // 4


@pytest.fixture(scope="module")
def ctxs():
    """one context per entry of CONFIGS; the environment is read at creation and restored afterwards"""
    import bulletproofspp_amd as b
    keys = ("BPPP_SCATTER_ONE_READ", "BPPP_HIST_CH", "BPPP_SORT_RANGES")
    old = {k: os.environ.get(k) for k in keys}
    out = []
    try:
        os.environ.pop("BPPP_SORT_RANGES", None)
        for one, ch in CONFIGS:
            os.environ["BPPP_SCATTER_ONE_READ"] = one
            if ch is None:
                os.environ.pop("BPPP_HIST_CH", None)
            else:
                os.environ["BPPP_HIST_CH"] = ch
            out.append(b.Bppp(0))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield out
    for g in out:
        g.close()


@pytest.fixture(scope="module")
def base_points():
    return points_to_array(O.hash_points(b"scatter one read", NBASE))


def _points(base_points, n):
    return np.ascontiguousarray(base_points[np.arange(n) % NBASE])


def _oracle(ec, base_points, sc, inf=()):
    """the oracle's MSM of the scalars (n, 4) uint64 over base point i mod 256, as 256 terms; `inf`: indices whose point is infinity"""
    sc = np.array(sc, dtype=np.uint64)
    sc[list(inf)] = 0
    n = sc.shape[0]
    pad = np.zeros((-(-n // NBASE) * NBASE, 4), dtype=np.uint64)
    pad[:n] = sc
    lo = (pad & np.uint64(0xFFFFFFFF)).reshape(-1, NBASE, 4).sum(axis=0)      # at most 2^20 / 256 rows of 32-bit halves: no overflow
    hi = (pad >> np.uint64(32)).reshape(-1, NBASE, 4).sum(axis=0)
    tot = [sum((int(lo[k, l]) + (int(hi[k, l]) << 32)) << (64 * l) for l in range(4)) % O.N for k in range(NBASE)]
    s = np.ascontiguousarray(scalars_to_array(tot))
    p = np.ascontiguousarray(base_points)
    return ec.inner_product_raw(s.ctypes.data_as(U64P), p.ctypes.data_as(U64P), NBASE)


def _random_scalars(n, seed):
    rnd = np.random.default_rng(seed)
    sc = rnd.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rnd.integers(0, 2, size=(n, 4), dtype=np.uint64)
    # all are < N (its top limb is 2^64 - 1); about half are over N / 2 and are folded (sign mask bits set); the others are >= 2^254, so
    # the top window's digit, whose row is stored negated, is not zero
    sc[:, 3] = (sc[:, 3] | np.uint64(1 << 62)) & np.uint64(0xFFFFFFFF00000000)
    return sc


def _hooks(g):
    from bulletproofspp_amd.capi import load_test_library
    lib = load_test_library()
    q, one = ctypes.c_int(-2), ctypes.c_int(-2)
    assert lib.bppp_test_last_sort_ranges(g.h, ctypes.byref(q)) == 0
    assert lib.bppp_test_last_scatter_one_read(g.h, ctypes.byref(one)) == 0
    return q.value, one.value


def _run_all(ctxs, sc, pts, window_bits, forced_chunk=False):
    """the MSM on the contexts without (or with) the forced chunk count; every one ran the ranged scatter with 4 ranges, and the form that
    make_plan's rule gives (_reads_once), if the context allows it"""
    n = sc.shape[0]
    out = []
    for (one, ch), g in zip(CONFIGS, ctxs):
        if (ch is not None) != forced_chunk:
            continue
        ds, dp = g.to_device(sc), g.to_device(pts)
        try:
            out.append(g.msm_device(ds, dp, n, window_bits=window_bits))
        finally:
            g.free(ds); g.free(dp)
        assert _hooks(g) == (4, 1 if one == "1" and _reads_once(n, ch) else 0), (one, ch, n, _hooks(g))
    return out


def _check(got, want):
    assert got[1] == want, "k_scatter_ranges against the oracle"
    assert got[0] == got[1], "BPPP_SCATTER_ONE_READ=1 against 0"


# n, window_bits, forced chunks, steps per lane and the form that the docstring derives
SIZES = [(200000, 0, False, 4, False), ((15 << 15) + 1, 0, False, 4, True), (17 << 15, 0, False, 4, False), (1 << 20, 0, False, 4, True),
         ((1 << 20) + 1, 0, False, 5, False), (1, 16, True, 1, True), (1 << 19, 16, True, 4, True), ((1 << 19) + 1, 16, True, 5, False)]


@pytest.mark.parametrize("n,window_bits,forced,steps,once", SIZES)
def test_sizes(ctxs, oracle_lib, base_points, n, window_bits, forced, steps, once):
    assert _chunks(n, FORCED if forced else None)[2] == steps and _reads_once(n, FORCED if forced else None) == once
    sc = _random_scalars(n, 50 + n % 97)
    _check(_run_all(ctxs, sc, _points(base_points, n), window_bits, forced), _oracle(oracle_lib, base_points, sc))


def test_below_the_smallest_size_the_plan_keeps_narrow_windows(ctxs, oracle_lib, base_points):
    """199 999 terms: 13-bit windows, k_scatter, on either context"""
    n = 199999
    sc = _random_scalars(n, 49)
    pts = _points(base_points, n)
    want = _oracle(oracle_lib, base_points, sc)
    for g in ctxs[:2]:
        ds, dp = g.to_device(sc), g.to_device(pts)
        try:
            assert g.msm_device(ds, dp, n) == want
        finally:
            g.free(ds); g.free(dp)
        assert _hooks(g) == (0, 0)


N_PAT = 70001          # window_bits = 16 and 16 forced chunks: 4376 digits each (one step for 547 lanes), the last one 4361; else 3 chunks


def _from_digits(rnd, lo, hi, top):
    """N_PAT scalars below N / 2 whose 16-bit window values are in [lo, hi] (below 2^15: no carries, the digit is the value), with `top` +
    (0 .. 6) in window 15"""
    d = rnd.integers(lo, hi + 1, size=(N_PAT, 16), dtype=np.uint64)
    d[:, 15] = np.uint64(top) + np.arange(N_PAT, dtype=np.uint64) % np.uint64(7)
    return sum(d[:, l::4] << np.uint64(16 * l) for l in range(4)).astype(np.uint64)     # limb j holds digits 4 j .. 4 j + 3


def _pattern(name):
    rnd = np.random.default_rng(51)
    if name == "range_0_only":
        # every digit of windows 0 .. 14 in bucket range 0 of 4 (|digit| <= 2^13): the passes of ranges 1 .. 3 place the top row's entries only
        return _from_digits(rnd, 1, 1 << 13, 0x6000)
    if name == "below_2_14":
        # the scalars themselves below 2^14: window 0 alone has entries, in ranges 0 and 1
        sc = np.zeros((N_PAT, 4), dtype=np.uint64)
        sc[:, 0] = rnd.integers(0, 1 << 14, size=N_PAT, dtype=np.uint64)
        return sc
    if name == "last_range":
        return _from_digits(rnd, (3 << 13) + 1, (1 << 15) - 1, 0x7000)
    if name == "one_scalar":
        # one bucket per window takes every entry
        return np.repeat(_random_scalars(1, 53), N_PAT, axis=0)
    # top digit 2^15, the largest there is: v in [2^255 - 2^239, (N - 1) / 2], as v and as N - v
    half = (O.N - 1) // 2
    r = random.Random(54)
    return scalars_to_array([(lambda v, i: v if i % 2 else O.N - v)(half - r.randrange(1 << 200), i) for i in range(N_PAT)])


@pytest.mark.parametrize("name", ["range_0_only", "below_2_14", "last_range", "one_scalar", "top_digit_max"])
def test_scalar_patterns(ctxs, oracle_lib, base_points, name):
    sc = _pattern(name)
    pts = _points(base_points, N_PAT)
    want = _oracle(oracle_lib, base_points, sc)
    _check(_run_all(ctxs, sc, pts, 16, forced_chunk=True), want)
    _check(_run_all(ctxs, sc, pts, 16), want)                        # 3 chunks, 48 workgroups: k_scatter_ranges on both


def test_zeros_and_infinity_at_the_chunk_borders(ctxs, oracle_lib, base_points):
    """zero scalars and points at infinity on both sides of chunk borders (16 forced chunks), at the ends of the input and of the last chunk"""
    n = N_PAT
    ch, per, _ = _chunks(n, FORCED)
    assert (ch, per) == (16, 4376) and _reads_once(n, FORCED)
    sc = _random_scalars(n, 52)
    pts = _points(base_points, n).copy()
    zero = [0, 7, 8, per - 8, per - 1, per, 2 * per - 1, 2 * per, 2 * per + 7, 15 * per - 1, 15 * per, n - 2, n - 1]
    inf = [1, 7, 9, per - 1, per, per + 1, 2 * per - 8, 2 * per, 15 * per, n - 1]
    sc[zero] = 0
    pts[inf] = 0                                              # affine (0, 0): infinity
    want = _oracle(oracle_lib, base_points, sc, inf)
    _check(_run_all(ctxs, sc, pts, 16, forced_chunk=True), want)
    _check(_run_all(ctxs, sc, pts, 16), want)
