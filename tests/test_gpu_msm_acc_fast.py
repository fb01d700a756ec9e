"""k_acc_points_sized29_fast (csrc/msm.hip section 3'; MsmTune::acc_fast, BPPP_ACC_FAST): the sized accumulation whose additions (affine + affine for
the first two finite entries, then the exception-free mixed addition) test nothing, with
one zero test of ZZ per item and the redo of a flagged item by the complete loop.  Whole MSMs on points with KNOWN DISCRETE LOGS, in the shape of
test_gpu_msm_acc_known_logs (whose cases, replay and launch this file reuses): every bucket is built by hand from one aligned group of 8 consecutive
terms, which one lane of the scatter places in index order, so that what the running sum meets, and where, is certain:
  items of 1, 2 and 3 entries;
  P = Q against the running sum at entries (0, 1), at (1, 2), in the middle and as the last entry;
  P = -Q at the same positions, among them buckets whose sum is infinity, and P = -Q followed by further entries (the sum restarts from infinity);
  the input point (0, 0) first, in the middle, last, and buckets of nothing else;
  equal y under different x (R = 0: no exception);
  buckets of ACC_CAP + 1 entries (two pieces, joined by k_merge_heavy<true>) with the exception inside the first piece, with a one-entry last
  piece that is opposite or equal to the first piece's sum or the point (0, 0), and with a first piece of (0, 0) points only.
Each case runs on a context created with BPPP_ACC_FAST=0 (k_acc_points_sized29, the complete addition in every step) and on one with the switch on:
the replay of the order the scatter produced reaches every class the case is built for, every bucket is bit for bit (log) G as an affine point
on both (the stored limbs of a sum are one of several representations of the same residue, so the `buckets` stage is compared as points), every
limb an item stores is below 2^26 with ZZ all zero exactly for infinity, and the final point is (sum s_i k_i) G and the same 64 bytes on both.
One seeded uniform MSM per window width against the CPU oracle, switch on and off, ends the file."""
import collections
import ctypes
import random

import numpy as np
import pytest

import msm_stages as S
import pyoracle as O
from bulletproofspp_amd.capi import TestMsmLayout, load_test_library, points_to_array, scalars_to_array
from test_gpu_msm_acc_known_logs import CAP, M_SIZED, Build, Case, E, N, _entry_log, _fmt, _lam, _launch, _madd, multiples  # noqa: F401  (multiples: a fixture)

pytestmark = pytest.mark.gpu

C = 13                                       # explicit window width: keeps a small input off the one-launch route (BPPP_ACC_SIZED=1 selects the sized route)
FAST = ("0", "1")
U64P = ctypes.POINTER(ctypes.c_uint64)


def _env(fast):
    return E(BPPP_ACC_SIZED=1, BPPP_ACC_FQ29=1, BPPP_HIST_CH=2, BPPP_ACC_FAST=fast)


def _buckets():
    """(entries, what the replay must call the additions of this bucket): an entry is (log, through the sign fold); 0 is the point (0, 0)"""
    a, b, d, e, g = 3, 10, 25, 57, 121                              # every partial sum differs from every later entry unless written so
    s2, s3, s4 = a + b, a + b + d, a + b + d + e
    rnd = random.Random(15)
    f = lambda *ks: [(k, rnd.random() < 0.3) for k in ks]
    return [
        (f(a), ()), (f(a, b), ("gen",)), (f(a, b, d), ("gen", "gen")),
        # P = Q
        (f(a, a), ("dbl1",)), (f(a, a, b), ("dbl1", "gen")), (f(a, b, s2), ("gen", "dblz")), (f(a, b, d, s3, e, g), ("gen", "gen", "dblz", "gen", "gen")),
        (f(a, b, d, e, s4), ("gen", "gen", "gen", "dblz")), (f(a, a, 2 * a, 4 * a), ("dbl1", "dblz", "dblz")),
        # P = -Q
        (f(a, -a), ("neg1",)), (f(a, -a, b), ("neg1", "ainf")), (f(a, b, -s2), ("gen", "negz")), (f(a, b, -s2, d, e), ("gen", "negz", "ainf", "gen")),
        (f(a, b, d, -s3, e, g), ("gen", "gen", "negz", "ainf", "gen")), (f(a, b, d, e, -s4), ("gen", "gen", "gen", "negz")),
        (f(a, -a, b, -b), ("neg1", "ainf", "neg1")), (f(a, a, -2 * a, b, b), ("dbl1", "negz", "ainf", "dbl1")),
        # the point (0, 0)
        (f(0), ()), (f(0, 0), ("qinf",)), (f(0, 0, 0), ("qinf", "qinf")), (f(0, a), ("ainf",)), (f(a, 0), ("qinf",)), (f(0, a, b), ("ainf", "gen")),
        (f(a, 0, b), ("qinf", "gen")), (f(a, b, 0), ("gen", "qinf")), (f(0, a, a), ("ainf", "dbl1")), (f(a, 0, -a), ("qinf", "neg1")),
        (f(0, 0, a, b, 0, s2, 0), ("qinf", "ainf", "gen", "qinf", "dblz", "qinf")), (f(a, 0, -a, 0, b), ("qinf", "neg1", "qinf", "ainf")),
        # equal y, different x
        (f(a, _lam(a)), ("samey",)), (f(a, b, _lam(s2), d), ("gen", "samey", "gen")),
        (f(a, b, d, e, g, 7, 11, s4 + g + 18), ("gen",) * 6 + ("dblz",)),
    ]


def _pieces(bd):
    """buckets of ACC_CAP + 1 entries: chunk 0 of the sort brings the first piece, its last chunk the one-entry second piece.  Equal entries double at
    (0, 1) in any order; a and -a in equal numbers double or cancel at (0, 1) and end in infinity in any order; distinct logs far above their count
    never meet a partial sum"""
    for first, last in (([2] * CAP, -2 * CAP), ([2] * CAP, 2 * CAP), ([2] * CAP, 0), ([2] * CAP, 7), ([5, -5] * (CAP // 2), 9), ([0] * CAP, 4), ([0] * CAP, 0),
                        ([1000 + i for i in range(CAP)], sum(1000 + i for i in range(CAP))), ([1000 + i for i in range(CAP)], -sum(1000 + i for i in range(CAP))),
                        ([0] + [3] * (CAP - 1), 0)):
        bucket = bd.fresh()
        for k in first:
            bd.term(0, [bucket], k)
        bd.term(bd.CH - 1, [bucket], last)


def _case(fast):
    fmt = _fmt(C, 1, False)
    bd = Build(fmt, 2)
    _pieces(bd)
    classes = []
    for _ in range(2):
        for entries, _cls in _buckets():
            classes.append((bd.fresh(), _cls))
            bd.group(0, classes[-1][0], entries)
    row, logs, _ = bd.finish()
    must = M_SIZED | {("sized.load", "inf"), ("sized.load", "pt"), ("order", "whole"), ("order", "pieces, the last short")} | \
        {("sheavy.tree", x) for x in ("gen", "dbl", "neg", "rinf", "linf")}
    return Case(f"acc_fast {fast}", "msm", C, _env(fast), [row], logs, 1, None, must), classes


@pytest.fixture(scope="module")
def contexts(gpu):
    made = S.make_contexts(gpu, [_env(v) for v in FAST])
    yield made
    S.close_contexts(made)


def _acc_fast(g):
    rep = TestMsmLayout()
    assert load_test_library().bppp_test_last_msm_layout(g.h, ctypes.byref(rep)) == 0
    return rep.acc_fast


def _point_words(p):
    return np.zeros(16, dtype=np.uint32) if p is None else np.frombuffer(p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little"), dtype=np.uint32)


@pytest.fixture(scope="module")
def hand_built(contexts, multiples):
    """per switch value: (case, classes, the sort's count and start, its order, affine buckets, raw buckets, final point), each MSM launched once"""
    out = {}
    for v in FAST:
        x, classes = _case(v)
        g = contexts[x.env]
        final = _launch(g, x, multiples)[0]
        lay = S.layout(g)
        assert S.hooks(g)[2:] == (1, 1) and bool(_acc_fast(g)) == (v != "0")
        out[v] = (x, classes, (S.read(g, lay, "count"), S.read(g, lay, "start")), S.read(g, lay, "sorted"), S.read(g, lay, "aff"), S.read(g, lay, "raw"), final)
    return out


@pytest.mark.parametrize("fast", FAST)
def test_hand_built_buckets(hand_built, multiples, fast):
    x, classes, (got_count, got_start), order, aff, raw, final = hand_built[fast]
    fmt, P, count, start, canon, plog, ref = x.prepared()
    assert (got_count == count).all() and got_start.tolist() == start
    assert int(count.max()) == CAP + 1 and int((count == CAP + 1).sum()) == 10
    # the replay of the observed order: the reference sums (Case.replay asserts them), the classes of the case, and per hand-built bucket the class of every addition
    logs, ev = x.replay(order.tolist())
    assert not x.must - set(k for k in ev if ev[k]), sorted(x.must - set(ev), key=str)
    for (w, d), cls in classes:
        fb = w * fmt.M + d - 1
        ent = order[start[fb]:start[fb + 1]].tolist()
        assert len(ent) == len(cls) + 1
        k0 = _entry_log(plog, ent[0], lambda i: i)
        acc, seen = (None if k0 is None else (k0, False)), []
        for en in ent[1:]:
            one = collections.Counter()
            acc = _madd(one, "m", acc, _entry_log(plog, en, lambda i: i))
            seen.append(next(iter(one))[1])
        assert tuple(seen) == cls, (w, d, seen, cls)
    # every bucket bit for bit (log) G
    want = np.zeros((P["FB"], 16), dtype=np.uint32)
    for fb, k in logs.items():
        want[fb] = multiples(k)
    bad = np.flatnonzero((aff != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} buckets differ from (log) G, first {[(int(f), int(count[f]), logs.get(int(f))) for f in bad[:8]]}"
    inf = np.array([f for f, k in logs.items() if k is None], dtype=np.int64)
    assert inf.size >= 16 and not raw[inf, 20:30].any() and not raw[count == 0, 20:30].any()
    assert raw[np.flatnonzero((want != 0).any(axis=1)), 20:30].any(axis=1).all()
    assert (raw[count <= CAP] < (1 << 26)).all()
    k = sum(s * l for s, l in zip(x.rows[0], x.logs)) % N
    assert _point_words(final).tolist() == multiples(k or None).tolist()


def test_switch_on_and_off_agree(hand_built):
    off, on = hand_built["0"], hand_built[FAST[-1]]
    assert on[6] == off[6]                                           # the final 64 bytes
    assert (on[3] == off[3]).all() and (on[4] == off[4]).all()       # the same order in, the same points in every bucket
    for v in FAST[1:]:
        assert hand_built[v][6] == off[6] and (hand_built[v][4] == off[4]).all()


@pytest.mark.parametrize("c", (13, 16))
def test_uniform_msm_switch_on_and_off(contexts, oracle_lib, c):
    n = 3000
    rnd = random.Random(1500 + c)
    sc = np.ascontiguousarray(scalars_to_array([rnd.randrange(O.N) for _ in range(n)]))
    pts = np.ascontiguousarray(points_to_array(O.hash_points(b"acc fast", n)))
    want = oracle_lib.inner_product_raw(sc.ctypes.data_as(U64P), pts.ctypes.data_as(U64P), n)
    for v in FAST:
        g = contexts[_env(v)]
        ds, dp = g.to_device(sc), g.to_device(pts)
        try:
            got = g.msm_device(ds, dp, n, window_bits=c)
        finally:
            g.free(ds); g.free(dp)
        assert S.hooks(g)[2:] == (1, 1) and bool(_acc_fast(g)) == (v != "0")
        assert got == want, (c, v)
