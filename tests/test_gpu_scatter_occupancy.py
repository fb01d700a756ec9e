"""The sort kernels' loops with their loads one step ahead (k_hist, k_scatter, k_scatter_ranges; csrc/msm.hip): a lane loads the digits and
sign bits of its next steps (k_scatter_ranges: four) before it places the current step's eight entries, and `j < hi` guards every such load
or selects its address, so that none reads past the chunk's end.  The sizes
below are the smallest at which those loops change path: one entry, a last step with fewer than eight digits, ends that are no multiple of 8
or 64, a chunk shorter than one step (nothing is loaded ahead), a second step for a few lanes only (8200 at 1024 lanes, every size over 2048
at 256), and chunk borders inside a 16-byte group (forced odd chunk counts).

Every result of msm_device is compared with the oracle's (pyoracle.CEC().inner_product_raw) and with the same call on a context created
with BPPP_SORT_RANGES=0 (k_scatter in place of k_scatter_ranges; the environment is read once per context).  window_bits = 16 selects the
ranged scatter whatever n, window_bits = 13 k_scatter with 256 lanes.  The test hooks do not expose the sorted entries, so the group
elements are the check of the positions too."""
import ctypes
import os
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd.capi import points_to_array, scalars_to_array

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)
SIZES = [1, 7, 8, 9, 63, 64, 65, 1023, 1025, 8191, 8200]
# (BPPP_SORT_RANGES, BPPP_HIST_CH): the default plan, the comparison, and forced chunk counts (3: borders at no multiple of 64, chunks of
# 8200 shorter than a step of 1024 lanes; 2 at 20011 terms: a second step that ends inside the chunk)
CONFIGS = [(4, None), (0, None), (2, None), (4, "3"), (0, "3"), (4, "2")]


def _oracle(ec, sc, pts):
    sc, pts = np.ascontiguousarray(sc), np.ascontiguousarray(pts)
    return ec.inner_product_raw(sc.ctypes.data_as(U64P), pts.ctypes.data_as(U64P), sc.shape[0])


@pytest.fixture(scope="module")
def ctxs():
    """one context per entry of CONFIGS; the environment is read at creation and restored afterwards"""
    import bulletproofspp_amd as b
    old = {k: os.environ.get(k) for k in ("BPPP_SORT_RANGES", "BPPP_HIST_CH")}
    out = []
    try:
        for q, ch in CONFIGS:
            os.environ["BPPP_SORT_RANGES"] = str(q)
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
def inputs(oracle_lib):
    """max(SIZES) random scalars and points (256 hashed ones, repeated) and the oracle's MSM of every prefix in SIZES, computed once"""
    rnd = random.Random(41)
    nmax = max(SIZES)
    sc = scalars_to_array([rnd.randrange(O.N) for _ in range(nmax)])
    pts = np.ascontiguousarray(points_to_array(O.hash_points(b"scatter occupancy", 256))[np.arange(nmax) % 256])
    return sc, pts, {n: _oracle(oracle_lib, sc[:n], pts[:n]) for n in SIZES}


def _last_q(g):
    from bulletproofspp_amd.capi import load_test_library
    q = ctypes.c_int(-2)
    assert load_test_library().bppp_test_last_sort_ranges(g.h, ctypes.byref(q)) == 0
    return q.value


def _run_all(ctxs, sc_arr, pt_arr, c):
    """the MSM on every context with window_bits = c; at 16 bits each context reports the scatter it was created for, below that k_scatter"""
    n = sc_arr.shape[0]
    out = []
    for (q, _), g in zip(CONFIGS, ctxs):
        ds, dp = g.to_device(sc_arr), g.to_device(pt_arr)
        try:
            out.append(g.msm_device(ds, dp, n, window_bits=c))
        finally:
            g.free(ds); g.free(dp)
        assert _last_q(g) == (q if c == 16 else 0), (q, c, _last_q(g))
    return out


def _check(got, want):
    for cfg, r in zip(CONFIGS, got):
        assert r == want, cfg


@pytest.mark.parametrize("n", SIZES)
def test_ranged_scatter_sizes(ctxs, inputs, n):
    sc, pts, want = inputs
    _check(_run_all(ctxs, sc[:n], pts[:n], 16), want[n])


@pytest.mark.parametrize("n", SIZES)
def test_plain_scatter_sizes(ctxs, inputs, n):
    """k_scatter and k_hist with 256 lanes: a step is 2048 digits, so 8191 and 8200 take four and five steps"""
    sc, pts, want = inputs
    _check(_run_all(ctxs, sc[:n], pts[:n], 13), want[n])


def test_second_step_ends_inside_the_chunk(ctxs, oracle_lib, inputs):
    """20011 terms: one chunk of 1024 lanes takes three steps, the last one for 454 lanes and with 3 valid digits in its last group; two
    chunks (10008 and 10003 digits) take two steps, the second for 227 lanes"""
    n = 20011
    rnd = random.Random(42)
    sc = scalars_to_array([rnd.randrange(O.N) for _ in range(n)])
    pts = np.ascontiguousarray(inputs[1][np.arange(n) % 256])
    _check(_run_all(ctxs, sc, pts, 16), _oracle(oracle_lib, sc, pts))


def _top_digit(s):
    """the signed 16-bit digit of the folded scalar in the top row (csrc/recode.hip.h): window value u >= 2^15 becomes u - 2^16 and carries"""
    v = min(s, O.N - s)
    return (v >> 240) + ((v >> 239) & 1)


def _patterns():
    n = 1025
    rnd = random.Random(43)
    equal = [rnd.randrange(O.N)] * n
    zero = [0] * n
    # top digit 2^15, the largest there is: v in [2^255 - 2^239, (N - 1) / 2], as v and as N - v
    half = (O.N - 1) // 2
    top = []
    for i in range(n):
        v = half - rnd.randrange(1 << 200) if i % 3 else half - i
        top.append(v if i % 2 else O.N - v)
    assert all(_top_digit(s) == 1 << 15 for s in top)
    # s > N / 2 for two thirds of the scalars, in runs that do not line up with the 8-entry groups or the mask's bytes
    neg = []
    for i in range(n):
        s = rnd.randrange(1, half)
        neg.append(O.N - s if (i * 5) % 13 % 3 else s)
    assert sum(s > half for s in neg) > n // 2
    return {"equal": equal, "zero": zero, "top_digit_max": top, "negated": neg}


@pytest.mark.parametrize("name", ["equal", "zero", "top_digit_max", "negated"])
def test_scalar_patterns(ctxs, oracle_lib, inputs, name):
    """all scalars equal (one bucket per window takes every entry), all zero (nothing is placed), the top row's digit at its maximum (that row
    is stored negated and the scatter flips its sign), and mostly scalars over N / 2 (negmask bits set)"""
    sc = scalars_to_array(_patterns()[name])
    pts = inputs[1][:sc.shape[0]]
    want = _oracle(oracle_lib, sc, pts)
    _check(_run_all(ctxs, sc, pts, 16), want)
    _check(_run_all(ctxs, sc, pts, 13), want)


def test_batch_sign_bits_straddle_mask_words(ctxs, oracle_lib, inputs):
    """3 instances of 9 terms through k_scatter: instance i starts at bit 9 i of the sign mask, so the eight sign bits of a step are not one
    byte (the m0 / m1 path); 3 of 57, where instance 1's first step takes bits 57 .. 64, the end of one 64-bit word and the start of the next;
    3 of 65, where instance 1's last full step (bits 121 .. 128) does"""
    rnd = random.Random(44)
    for n in (9, 65, 57):
        batch = 3
        sc = [[rnd.randrange(O.N) for _ in range(n)] for _ in range(batch)]
        for s in sc:                       # every other scalar is over N / 2: set and clear bits alternate across the word borders
            for i in range(0, n, 2):
                s[i] = O.N - s[i] if s[i] < O.N // 2 else s[i]
        sarr = np.concatenate([scalars_to_array(s) for s in sc])
        parr = np.ascontiguousarray(inputs[1][:n])
        want = [_oracle(oracle_lib, scalars_to_array(s), parr) for s in sc]
        for cfg, g in zip(CONFIGS, ctxs):
            ds, dp = g.to_device(sarr), g.to_device(parr)
            try:
                for c in (13, 16):
                    assert g.msm_batch_device(ds, dp, n, batch, shared_points=True, window_bits=c) == want, (cfg, n, c)
                    assert _last_q(g) == 0
            finally:
                g.free(ds); g.free(dp)
