"""The bucket reductions and window combines of csrc/msm.hip on points with KNOWN DISCRETE LOGS, so that bucket sums, running sums, row sums and
block sums can be made equal or opposite on purpose: the doubling and the cancelling branch of the complete additions inside k_reduce1 / k_reduce2,
k_reduce_groups, k_reduce_marg, both steps of k_reduce_tail_quad, the tail of k_msm_small, k_msm_small_join and k_window_combine.  (With hashed
points the sums of two buckets are unrelated.  Equal partial sums then meet only where the sum of one sparse bucket reaches a tree twice, as the
suffix of several lanes; the suffix scans, the serial loops, the lines that join wavefronts and slices, the combine, and the cancelling branch
nearly everywhere, are not reached that way.)

Reference, shared with nothing in the library: every point is k_i G with a small signed k_i the test knows (k = 0: the infinity point), so an
instance's result is (sum s_i k_i mod n) G - Python integers and one oracle scalar multiplication - or None when the sum is 0 mod n.  Every instance
of every launch is compared bit for bit; a few small cases also with the oracle's innerProduct over the points themselves.

The digit format (csrc/recode.hip.h, window_layout of csrc/msm_plan.hpp: balanced and uniform widths, the unbiased top row stored negated) is
restated in Fmt, with its inverse: a term (d * 2^off_w, b G) puts the log b into bucket d - 1 of window w alone, and one scalar with the digit d in
every window fills that bucket everywhere.  The buckets a case fills are DERIVED from its scalars by the forward restatement, never assumed.

The unmarked tests replay every reduction kernel lane for lane on integers (discrete logs in place of points, None for infinity) and classify
every addition by the branch it takes (rinf / linf: the right / left operand is infinity, gen, dbl: P = Q, neg: P = -Q) and every doubling by
whether its input is infinity.  The replay of a case ends in the case's plain reference value, which checks the weighted-sum identities (for the
marginal route LO * W1 + W2 = sum (i + 1) B_i) and the restated format together; the union of the counts over the case list must contain every
branch of every loop (LOOPS), except the pairs listed in UNREACHABLE with the reason why no input gets there.

Each GPU test first asserts the route and geometry the library reports (bppp_test_last_reduce) against literals; the plan arithmetic that yields
them is restated in _plan / _small_plan and compared with the same literals on the CPU."""
import collections
import ctypes
import functools
import random

import numpy as np
import pytest

import pyoracle as O

N = O.N
HALF = (N - 1) // 2
G = (O.GX, O.GY)
SMALL, GROUPS, MARG, WAVE = 0, 1, 2, 3                              # bppp_test_reduce_report.route
FIELDS = ("route", "combine", "c", "W", "M", "RG", "Lw", "WPW", "a", "LO", "HI", "PR", "PC", "SR", "SC", "TR", "TC", "S")
BRANCHES = ("rinf", "linf", "gen", "dbl", "neg")


def _lit(route, c, W, combine=0, **kw):
    d = dict.fromkeys(FIELDS, 0)
    d.update(route=route, combine=combine, c=c, W=W, M=1 << (c - 1), **kw)
    return d


# ----------------------------------------------------------------------------- the digit format, restated (and its inverse)
def _layout(c, balanced):
    """window_layout: (W, acnt, top)"""
    if balanced:
        W = -(-256 // c)
        return W, 256 - W * (c - 1), W - 1
    T = -(-255 // c)
    r = 255 - c * (T - 1)
    W = T + (1 if r == c else 0)
    return W, W, (W - 1 if r == c - 1 else -1)


class Fmt:
    """the signed digits of a scalar as the kernels read them: windows [0, acnt) are c bits wide, the others c - 1; every window is biased by half its
    range except an unbiased top one, whose non-negative digit is stored negated and its entries' signs flipped"""

    def __init__(self, c, W, acnt, top):
        self.c, self.W, self.acnt, self.top, self.M = c, W, acnt, top, 1 << (c - 1)
        self.cw = [c if w < acnt else c - 1 for w in range(W)]
        self.off = [sum(self.cw[:w]) for w in range(W)]
        self.K = sum(1 << (self.off[w] + self.cw[w] - 1) for w in range(W) if w != top)
        self._memo = {}

    def digits(self, s):
        """per window the signed digit e (0: no entry): the entry goes to bucket |e| - 1 and adds sign(e) * P"""
        if s in self._memo:
            return self._memo[s]
        neg = s > N - s
        v = N - s if neg else s
        sp, out = v + self.K, []
        for w in range(self.W):
            cw = self.cw[w]
            f = sp & ((1 << cw) - 1)
            sp >>= cw
            if w == self.top:
                stored, flip = self.M - f, 1                        # k_digits: 2^(c-1) - d
            else:
                stored, flip = f + (0 if w < self.acnt else 1 << (self.c - 2)), 0
            assert 0 <= stored < 1 << 16
            kv = stored - self.M                                    # what every consumer reads
            assert abs(kv) <= 1 << (cw - 1)                         # a narrow window reaches the lower half of the buckets only
            minus = (kv < 0) ^ neg ^ flip
            out.append(-abs(kv) if minus else abs(kv))
        assert sp == 0 and sum(e << o for e, o in zip(out, self.off)) == (-v if neg else v)
        self._memo[s] = out
        return out

    def scalar(self, d, w=None):
        """the inverse: the scalar whose digit is d in window w alone (w given; d = 2^(cw-1) of a biased window becomes -d there and a carry of 1
        into the window above), or in every window that can hold it without the scalar leaving [0, (n - 1) / 2] (w None)"""
        if w is not None:
            s = d << self.off[w]
            assert 0 < d <= 1 << (self.cw[w] - 1) and s <= HALF
            return s
        s = 0
        for x in range(self.W):
            lim = (1 << (self.cw[x] - 1)) - (0 if x == self.top else 1)
            if d <= lim and s + (d << self.off[x]) <= HALF:
                s += d << self.off[x]
        return s


@functools.lru_cache(maxsize=None)
def _fmt(c, batch, flat):
    if flat:
        return Fmt(c, 256 // c + 1, 256 // c + 1, -1)               # a registered basis: 256 / c + 1 biased rows of c bits
    return Fmt(c, *_layout(c, batch == 1 and c >= 3 and 256 % c != 0))


def _buckets(fmt, scalars, logs, flat):
    """the bucket sums, as logs mod n: [window][M], or [1][M] with the table's 2^off_w folded in when all windows share one bucket set"""
    B = [[0] * fmt.M for _ in range(1 if flat else fmt.W)]
    for s, k in zip(scalars, logs):
        if s and k:
            for w, e in enumerate(fmt.digits(s)):
                if e:
                    B[0 if flat else w][abs(e) - 1] += (k if e > 0 else -k) << (fmt.off[w] if flat else 0)
    return [tuple(x % N or None for x in row) for row in B]


# ----------------------------------------------------------------------------- the plan arithmetic, restated
def _plan(c, batch, flat=False, lw=0, rg=0, marg_s=0):
    """plan_windows + plan_reduce of csrc/msm_plan.hpp and msm_finish's choice of the combine, as the report names them"""
    fmt = _fmt(c, batch, flat)
    M, NS = fmt.M, batch * (1 if flat else fmt.W)
    FB = NS * M
    r = _lit(WAVE, c, 1 if flat else fmt.W, combine=int(batch > 4))
    Lw = 1
    if M > 64:
        while M // Lw > 4096:
            Lw <<= 1
        if M // Lw >= 1024 and Lw < 4:
            Lw = min(4, M // 1024)
        if lw and lw & (lw - 1) == 0 and 64 <= M // lw <= 4096:
            Lw = lw
    WPW = max(1, M // Lw // 64)
    RG = 0
    if M <= 256 and NS >= 4096:
        cap = min(8, M)
        RG = max(1, min(cap, M // 16))
        while RG < cap and NS * RG < 131072:
            RG <<= 1
        if 1 <= rg <= cap and rg & (rg - 1) == 0:
            RG = rg
    if RG:
        r.update(route=GROUPS, RG=RG, Lw=M // RG)
    elif M >= 256 and NS <= 65535:
        a = c // 2
        LO = 1 << a
        HI = M // LO
        S = 1
        while S < 16 and 2.0 * FB / S > 98304.0:
            S <<= 1
        if 1 <= marg_s <= 64 and marg_s & (marg_s - 1) == 0:
            S = marg_s
        SR, SC = min(S, LO), min(S, HI)
        PR, PC = LO // SR, HI // SC
        while PR > 64:
            PR, SR = PR >> 1, SR << 1
        while PC > 64:
            PC, SC = PC >> 1, SC << 1
        r.update(route=MARG, a=a, LO=LO, HI=HI, PR=PR, PC=PC, SR=SR, SC=SC, TR=HI // 16, TC=LO // 16)
    else:
        r.update(Lw=Lw, WPW=WPW)
    return r


def _small_plan(n, small_c=0, small_len=0):
    """make_small_plan"""
    c = small_c if 5 <= small_c <= 8 else 6
    ln = small_len if 64 <= small_len <= 4096 else (512 if n <= 2048 else 1024)
    if n <= ln + ln // 2:
        ln = n
    return _lit(SMALL, c, _fmt(c, 1, False).W, S=-(-n // ln)), ln


# ----------------------------------------------------------------------------- the replay: integer "points" and the complete addition's branches
def _add(ev, loop, a, b):
    """acc += q as xyzz_add / xyzz_add_chain / xyzz_add_quad decide it"""
    if b is None:
        ev[loop, "rinf"] += 1
        return a
    if a is None:
        ev[loop, "linf"] += 1
        return b
    if a == b:
        ev[loop, "dbl"] += 1
        return 2 * a % N
    if a + b == N:
        ev[loop, "neg"] += 1
        return None
    ev[loop, "gen"] += 1
    return (a + b) % N


def _dbl(ev, loop, a):
    ev[loop, "dinf" if a is None else "dpt"] += 1
    return None if a is None else 2 * a % N


def _scan_tree(ev, name, run, acc, Lw, width):
    """the cross-lane part k_reduce1, k_reduce_groups and k_reduce2 share: inclusive suffix scan of `run` over `width` lanes, the lanes >= 1 keep
    their suffix, times Lw by doublings, plus acc, then the tree.  Returns (lane 0's value, lane 0's suffix)"""
    suf = list(run)
    d = 1
    while d < width:
        suf = [_add(ev, name + ".scan", suf[l], suf[l + d]) if l + d < width else suf[l] for l in range(width)]
        d <<= 1
    v = [suf[l] if l >= 1 else None for l in range(width)]
    k = Lw
    while k > 1:
        v = [_dbl(ev, name + ".ladder", x) for x in v]
        k >>= 1
    v = [_add(ev, name + ".addacc", v[l], acc[l]) for l in range(width)]
    d = width >> 1
    while d >= 1:
        v = [_add(ev, name + ".tree", v[l], v[l + d]) if l + d < width else v[l] for l in range(width)]
        d >>= 1
    return v[0], suf[0]


def _serial(ev, name, B, t, Lw):
    run = acc = None
    for k in range(Lw - 1, -1, -1):
        run = _add(ev, name + ".serial_run", run, B[t * Lw + k])
        acc = _add(ev, name + ".serial_acc", acc, run)
    return run, acc


def _m_wave(ev, B, Lw, WPW):
    """k_reduce1 (one wavefront per 64 * Lw buckets) + k_reduce2"""
    M, red = len(B), []
    for wave in range(WPW):
        lanes = [_serial(ev, "r1", B, wave * 64 + l, Lw) if (wave * 64 + l) * Lw < M else (None, None) for l in range(64)]
        red.append(_scan_tree(ev, "r1", [x[0] for x in lanes], [x[1] for x in lanes], Lw, 64))
    A = [red[l][0] if l < WPW else None for l in range(64)]
    S = [red[l][1] if l < WPW else None for l in range(64)]
    return _scan_tree(ev, "r2", S, A, 64 * Lw, 64)[0]


def _m_groups(ev, B, RG):
    Lw = len(B) // RG
    lanes = [_serial(ev, "rg", B, g, Lw) for g in range(RG)]
    return _scan_tree(ev, "rg", [x[0] for x in lanes], [x[1] for x in lanes], Lw if RG > 1 else 1, RG)[0]


def _m_marg_sums(ev, B, g):
    """k_reduce_marg: marg_serial_sum per lane, then the segmented tree; (R[HI], C[LO])"""
    LO, HI = g["LO"], g["HI"]

    def lane_sums(P, S, first, stride):
        out = []
        for part in range(P):
            acc = B[first(part)]
            for k in range(1, S):
                acc = _add(ev, "marg.serial", acc, B[first(part) + k * stride])
            out.append(acc)
        d = P >> 1
        while d >= 1:
            out = [_add(ev, "marg.tree", out[p], out[p + d]) if p + d < P else out[p] for p in range(P)]
            d >>= 1
        return out[0]
    R = [lane_sums(g["PR"], g["SR"], lambda part: hi * LO + part * g["SR"], 1) for hi in range(HI)]
    C = [lane_sums(g["PC"], g["SC"], lambda part: part * g["SC"] * LO + lo, LO) for lo in range(LO)]
    return R, C


def _m_tail(ev, E, nb):
    """k_reduce_tail_quad for one (window, kind): sum (i + 1) E_i over nb blocks of 16 quads, the second step by the last block"""
    part = []
    for b in range(nb):
        suf = list(E[16 * b:16 * b + 16])
        d = 1
        while d < 16:
            before = dict(ev)
            suf = [_add(ev, "tq.scan1", suf[q], suf[q + d] if q + d < 16 else None) for q in range(16)]
            # the control flow of xyzz_add_quad has three paths: doubling and cancelling leave early, everything else runs the generic body
            if all(ev[("tq.scan1", x)] > before.get(("tq.scan1", x), 0) for x in ("dbl", "neg")) and \
                    any(ev[("tq.scan1", x)] > before.get(("tq.scan1", x), 0) for x in ("gen", "linf", "rinf")):
                ev["tq.scan1", "three paths in one step"] += 1
            d <<= 1
        v = list(suf)
        d = 8
        while d >= 1:
            v = [_add(ev, "tq.tree1", v[q], v[q + d] if q + d < 16 else None) for q in range(16)]
            d >>= 1
        part.append((v[0], suf[0]))
    A = [part[q][0] if q < nb else None for q in range(16)]
    S = [part[q][1] if q < nb else None for q in range(16)]
    d = 1
    while d < nb:
        S = [_add(ev, "tq.scan2", S[q], S[q + d] if q + d < nb else None) for q in range(16)]
        d <<= 1
    v = [S[q] if q >= 1 else None for q in range(16)]
    for _ in range(4):
        v = [_dbl(ev, "tq.dbl2", x) for x in v]
    v = [_add(ev, "tq.addA", v[q], A[q]) for q in range(16)]
    d = nb >> 1
    while d >= 1:
        v = [_add(ev, "tq.tree2", v[q], v[q + d] if q + d < nb else None) for q in range(16)]
        d >>= 1
    return v[0]


def _m_marg(ev, B, g):
    R, C = _m_marg_sums(ev, B, g)
    W1 = _m_tail(ev, R[1:] + [None], g["TR"])                       # the R kind reads its elements shifted by one
    W2 = _m_tail(ev, C, g["TC"])
    assert ((W1 or 0) * g["LO"] + (W2 or 0)) % N == sum((i + 1) * (b or 0) for i, b in enumerate(B)) % N
    return W1, W2


def _m_small(ev, B):
    """the tail of k_msm_small from the M bucket sums on: suffix scan + tree per wavefront, then lane 0's A_0 + A_1 + 64 T_1"""
    M = len(B)
    Mw, res = min(M, 64), []
    for j in range(-(-M // 64)):
        suf = list(B[64 * j:64 * j + Mw])
        d = 1
        while d < Mw:
            suf = [_add(ev, "sm.scan", suf[l], suf[l + d]) if l + d < Mw else suf[l] for l in range(Mw)]
            d <<= 1
        v = list(suf)
        d = Mw >> 1
        while d >= 1:
            v = [_add(ev, "sm.tree", v[l], v[l + d]) if l + d < Mw else v[l] for l in range(Mw)]
            d >>= 1
        res.append((v[0], suf[0]))
    r = res[0][0]
    for a, t in res[1:]:
        for _ in range(6):
            t = _dbl(ev, "sm.dbl64", t)
        r = _add(ev, "sm.addA", r, a)
        r = _add(ev, "sm.addT", r, t)
    return r


def _m_small_join(ev, parts):
    """k_msm_small_join: lane l starts from slice l and adds slices l + 64, ...; then a tree over the next power of two"""
    S = len(parts)
    acc = [None] * 64
    for l in range(64):
        for s in range(l, S, 64):
            acc[l] = parts[s] if s < 64 else _add(ev, "smj.serial", acc[l], parts[s])
    top = 1
    while top < S and top < 64:
        top <<= 1
    d = top >> 1
    while d >= 1:
        acc = [_add(ev, "smj.tree", acc[l], acc[l + d]) if l + d < 64 else acc[l] for l in range(64)]
        d >>= 1
    return acc[0]


def _m_combine(ev, wins, c, a):
    """k_window_combine for one instance: wins[w] = t_w, or (W1, W2) with a > 0"""
    r = None
    for t in reversed(wins):
        if a:
            for _ in range(c - a):
                r = _dbl(ev, "wc.dbl", r)
            r = _add(ev, "wc.add1", r, t[0])
            for _ in range(a):
                r = _dbl(ev, "wc.dbl", r)
            r = _add(ev, "wc.add2", r, t[1])
        else:
            for _ in range(c):
                r = _dbl(ev, "wc.dbl", r)
            r = _add(ev, "wc.add", r, t)
    return r


_window_memo = {}


def _window(ev, rep, B):
    """one window's reduction by the route of `rep`, memoised on the bucket vector (many windows of a case are alike)"""
    key = (tuple(sorted(rep.items())), B)
    if key not in _window_memo:
        e = collections.Counter()
        if rep["route"] == WAVE:
            val = _m_wave(e, B, rep["Lw"], rep["WPW"])
        elif rep["route"] == GROUPS:
            val = _m_groups(e, B, rep["RG"])
        elif rep["route"] == MARG:
            val = _m_marg(e, B, rep)
        else:
            val = _m_small(e, B)
        if rep["route"] != MARG:
            assert (val or 0) == sum((i + 1) * (b or 0) for i, b in enumerate(B)) % N
        _window_memo[key] = (val, e)
    val, e = _window_memo[key]
    ev.update(e)
    return val


# ----------------------------------------------------------------------------- cases
class Case:
    """kind: 'small' (bppp_msm), 'msm' (bppp_msm_device with window_bits), 'batch' (bppp_msm_batch_device), 'basis' (Basis.msm).  rows: [batch][n]
    scalars; logs: [n], or [batch][n] with points per instance; env: the tuning the context is created under; want: the report literal"""

    def __init__(self, name, kind, c, rows, logs, want, env=(), slice_len=0):
        self.name, self.kind, self.c, self.rows, self.logs, self.want, self.env, self.slice_len = name, kind, c, rows, logs, want, env, slice_len
        self.batch, self.n, self.shared = len(rows), len(rows[0]), not isinstance(logs[0], (list, tuple))
        assert all(len(r) == self.n for r in rows) and all(0 <= s < N for r in rows for s in r)

    def logs_of(self, b):
        return self.logs if self.shared else self.logs[b]

    def reference(self):
        return [sum(s * k for s, k in zip(r, self.logs_of(b))) % N or None for b, r in enumerate(self.rows)]

    def fmt(self):
        return _fmt(self.c, self.batch, self.kind == "basis")

    @functools.lru_cache(maxsize=None)
    def replay(self):
        """(the result of every instance by the replay of the case's kernels, the branch counts)"""
        ev, fmt, rep, out = collections.Counter(), self.fmt(), self.want, []
        for b, row in enumerate(self.rows):
            if self.kind == "small":
                slices = [_buckets(fmt, row[j:j + self.slice_len], self.logs_of(b)[j:j + self.slice_len], False) for j in range(0, self.n, self.slice_len)]
                assert len(slices) == rep["S"]
                wins = [[_window(ev, rep, B) for B in sl] for sl in slices]
                wins = [_m_small_join(ev, [sl[w] for sl in wins]) if rep["S"] > 1 else wins[0][w] for w in range(fmt.W)]
            else:
                wins = [_window(ev, rep, B) for B in _buckets(fmt, row, self.logs_of(b), self.kind == "basis")]
            if rep["combine"]:
                out.append(_m_combine(ev, wins, self.c, rep["a"]))
            else:                                                   # the host's combine (tests/native/hostcurve_check.cpp): plain arithmetic here
                val = [(t[0] or 0) * rep["LO"] + (t[1] or 0) if rep["route"] == MARG else (t or 0) for t in wins]
                out.append(sum(v << (0 if self.kind == "basis" else fmt.off[w]) for w, v in enumerate(val)) % N or None)
        return out, ev


def _pad(rows, logs):
    n = max(len(r) for r in rows)
    rows = [list(r) + [0] * (n - len(r)) for r in rows]
    if isinstance(logs[0], (list, tuple)):
        logs = [list(l) + [1] * (n - len(l)) for l in logs]
    else:
        logs = list(logs) + [1] * (n - len(logs))
    return rows, logs


def _terms(fmt, spec, w=None, fold_every=0):
    """terms (scalar, log) that put log b into bucket m of window w (None: of every window that can hold the digit), for spec = {m: b}; every
    fold_every-th term goes in as (n - s, -b G): the same entry through the sign fold"""
    out = []
    for i, (m, b) in enumerate(sorted(spec.items())):
        if not b:
            continue
        s = fmt.scalar(m + 1, w)
        if s:
            out.append((N - s, -b) if fold_every and i % fold_every == 0 else (s, b))
    return out


# bucket patterns over `lim` buckets
def p_equal(lim):
    return {m: 1 for m in range(lim)}


def p_alt(lim):
    return {m: 1 if m % 2 == 0 else -1 for m in range(lim)}


def p_rand(lim, seed, vals=(0, 0, 1, -1, 2, -2)):
    rnd = random.Random(seed)
    return {m: rnd.choice(vals) for m in range(lim)}


P_ZERO_SUM = {0: 2, 1: -1, 2: -2, 5: 1}                             # 2 - 2 - 6 + 6: non-empty buckets whose weighted sum is infinity


def _ends(fmt, w, b=1):
    """only bucket 1 and bucket M of window w: the digit 2^(cw-1) of a biased window is stored as -2^(cw-1) with a carry into the window above, so
    the term (2^(cw-1) 2^off_w, b G) puts -b into bucket M of window w and b into bucket 1 of window w + 1"""
    return [(fmt.scalar(1 << (fmt.cw[w] - 1), w), b)]


def _one(kind, c, name, terms, want, env=(), **kw):
    rows, logs = _pad([[s for s, _ in terms]], [k for _, k in terms])
    return Case(name, kind, c, rows, logs, want, env, **kw)


def _second_step(fmt, LO, nbR, nbC):
    """marginal route, second step of k_reduce_tail_quad: a window whose buckets lie in row 0 alone has C_lo = B_lo and no R element the tail reads,
    one whose buckets lie in column 0 alone has R_hi = B_(hi LO); so the element vector E of either kind is chosen directly.  Per window and kind:
    blocks with equal sums S_b (second scan: doubling), alternating sums (cancelling), a last block with 16 S_b = A_b (add-A doubles) and with
    A_b = -16 S_b (add-A cancels), and v_0 = +-v_1 for the second tree"""
    terms, w = [], 0

    def put(kind, E):
        nonlocal w
        for i, b in E.items():
            terms.extend(_terms(fmt, {i if kind == "C" else (i + 1) * LO: b}, w))
        w += 1
    for kind, nb in (("R", nbR), ("C", nbC)):
        n = 16 * nb - (1 if kind == "R" else 0)                     # the R kind has HI - 1 elements
        last = 16 * (nb - 1)
        put(kind, {i: 1 for i in range(n)})
        put(kind, {i: 1 if (i // 16) % 2 == 0 else -1 for i in range(n)})
        if kind == "C":
            put(kind, {last + 15: 1, 3: 1})                         # A_b = 16 E_15 = 16 S_b
            put(kind, {last + 15: 17, last: -32, 5: 2})             # A_b = 16 * 17 - 32 = -16 (17 - 32)
        else:                                                       # the last R block has 15 elements: weights 1 .. 15
            put(kind, {last + 14: 2, last + 13: -1, 3: 1})          # A_b = 30 - 14 = 16 (2 - 1)
            put(kind, {last + 14: 17, last: -31, 5: 2})             # A_b = 15 * 17 - 31 = -16 (17 - 31)
        put(kind, {16: 1, 0: 17})
        put(kind, {16: 1, 0: -17})
    assert w <= fmt.acnt
    return terms


def _general_terms(fmt, seed, lim=None):
    """the patterns every route gets: over all windows at once - equal, alternating, random with a third empty (some through the sign fold), a
    weighted sum of zero - and single windows holding one pattern each while the pattern above is absent there"""
    lim = lim or fmt.M - 1
    return [("equal", _terms(fmt, p_equal(lim))), ("alt", _terms(fmt, p_alt(lim))), ("rand", _terms(fmt, p_rand(lim, seed), fold_every=3)),
            ("zero", _terms(fmt, P_ZERO_SUM)),
            ("single", _terms(fmt, p_equal(min(lim, (1 << (fmt.cw[1] - 1)) - 1)), 1) + _terms(fmt, p_alt(min(lim, (1 << (fmt.cw[fmt.W - 2] - 1)) - 1)), fmt.W - 2)
             + _ends(fmt, 2) + _terms(fmt, p_rand(min(lim, (1 << (fmt.cw[4 % fmt.W] - 1)) - 1), seed + 1), 4 % fmt.W))]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # ---- small route: c = 6, 43 windows (41 of 6 bits, 2 of 5), M = 32
    f6 = _fmt(6, 1, False)
    for name, terms in _general_terms(f6, 60):
        out.append(_one("small", 6, "small c6 " + name, (terms + [(0, 1)] * 64)[:max(64, len(terms))], _lit(SMALL, 6, 43, S=1), slice_len=max(64, len(terms))))
    # three slices of 1024, 1024 and 32 terms: identical, opposite, and the third equal or opposite to the first
    X = _terms(f6, p_rand(31, 61)) + _terms(f6, {3: 2}, 7)
    neg = lambda ts: [(s, -k) for s, k in ts]
    fill = lambda ts, n: ts + [(0, 1)] * (n - len(ts))
    for name, s0, s1, s2 in (("same same none", X, X, []), ("same opposite other", X, neg(X), _terms(f6, {1: 1})), ("first equals third", X, _terms(f6, {2: 1}), X),
                             ("first opposite third", X, [], neg(X))):
        out.append(_one("small", 6, "small three slices " + name, fill(s0, 1024) + fill(s1, 1024) + fill(s2, 32), _lit(SMALL, 6, 43, S=3), slice_len=1024))
    # BPPP_MSM_SMALL_LEN=64: 65 slices, lane 0 of the join adds slice 64 to slice 0 before the tree
    for name, s64 in (("equal", X), ("opposite", neg(X)), ("other", _terms(f6, {0: 1})), ("none", [])):
        body = fill(X, 64) + fill(_terms(f6, {4: 1}), 64) + [(0, 1)] * (62 * 64) + fill(s64, 64)
        out.append(_one("small", 6, "small 65 slices, the last " + name, body, _lit(SMALL, 6, 43, S=65), env=(("BPPP_MSM_SMALL_LEN", "64"),), slice_len=64))
    out.append(_one("small", 6, "small 65 slices, the first empty", [(0, 1)] * (64 * 64) + fill(X, 64), _lit(SMALL, 6, 43, S=65), env=(("BPPP_MSM_SMALL_LEN", "64"),), slice_len=64))
    # BPPP_MSM_SMALL_C=8: M = 128, two wavefronts, lane 0's A_0 + A_1 + 64 T_1 (A_j = sum (l + 1) B_(64 j + l), T_j = sum B_(64 j + l))
    f8 = _fmt(8, 1, False)
    env8 = (("BPPP_MSM_SMALL_C", "8"),)
    for name, terms in _general_terms(f8, 80) + [
            ("A0 = A1", _terms(f8, {0: 3, 64: 1, 65: 1})),                                      # A_1 = 1 + 2
            ("A0 = -A1", _terms(f8, {0: -3, 64: 1, 65: 1})),
            ("A1 empty, T1 not", _terms(f8, {0: 1, 64: 2, 65: -1})),                            # A_1 = 2 - 2, T_1 = 1
            ("A0 + A1 = 64 T1", _terms(f8, {0: 125, 64: 1, 65: 1})),                            # 125 + 3 = 128 = 64 * 2
            ("A0 + A1 = -64 T1", _terms(f8, {0: -131, 64: 1, 65: 1})),                          # -131 + 3 = -128 = -64 * 2
            ("A0 = -64 T1, A1 empty", _terms(f8, {0: -64, 64: 2, 65: -1}))]:
        out.append(_one("small", 8, "small c8 " + name, (terms + [(0, 1)] * 100)[:max(100, len(terms))], _lit(SMALL, 8, 32, S=1), env=env8, slice_len=max(100, len(terms))))
    # ---- wavefront route: one MSM with explicit window_bits
    for c, W, kw in ((2, 128, dict(Lw=1, WPW=1)), (5, 52, dict(Lw=1, WPW=1)), (7, 37, dict(Lw=1, WPW=1)), (8, 32, dict(Lw=1, WPW=2))):
        f = _fmt(c, 1, False)
        for name, terms in _general_terms(f, c) if c > 2 else [("all", _terms(f, {0: 1}) + _terms(f, {0: -1}, 5) + _ends(f, 9) + _ends(f, 10, -1))]:
            out.append(_one("msm", c, f"wave c{c} {name}", terms, _lit(WAVE, c, W, **kw)))
    # k_reduce2 on its two wavefronts (A_j = sum (l + 1) B_(64 j + l), S_j = sum B_(64 j + l)): A_0 = +-(64 S_1 + A_1) in the tree (S_1 = 2, A_1 = 3),
    # 64 S_1 = A_1 (2 * 63 - 62 = 64, S_1 = 1) and = -A_1 (127 - 65 * 63 = -64 * 62) in the addition of A, S_0 = +-S_1 in the scan
    for name, spec in (("v0 = v1", {0: 131, 64: 1, 65: 1}), ("v0 = -v1", {0: -131, 64: 1, 65: 1}), ("64 S1 = A1", {126: 2, 125: -1, 0: 1}), ("64 S1 = -A1", {64: 127, 126: -65}),
                       ("S0 = S1", {0: 1, 64: 1}), ("S0 = -S1", {0: 1, 64: -1})):
        out.append(_one("msm", 8, "wave c8 " + name, _terms(f8, spec), _lit(WAVE, 8, 32, Lw=1, WPW=2)))
    envlw = (("BPPP_LW", "2"),)
    for name, terms in _general_terms(f8, 82) + [("B0 = -2 B1", _terms(f8, {1: 1, 0: -2, 3: 2, 2: -2, 5: 1, 4: 1})), ("pairs", _terms(f8, {2 * i + (i & 1): 1 for i in range(64)}))]:
        out.append(_one("msm", 8, "wave c8 Lw2 " + name, terms, _lit(WAVE, 8, 32, Lw=2, WPW=1), env=envlw))
    # ---- marginal route: one MSM
    g9 = dict(a=4, LO=16, HI=16, PR=16, PC=16, SR=1, SC=1, TR=1, TC=1)
    g12 = dict(a=6, LO=64, HI=32, PR=64, PC=32, SR=1, SC=1, TR=2, TC=4)
    g13 = dict(a=6, LO=64, HI=64, PR=32, PC=32, SR=2, SC=2, TR=4, TC=4)
    g16 = dict(a=8, LO=256, HI=128, PR=16, PC=8, SR=16, SC=16, TR=8, TC=16)
    for c, W, g in ((9, 29, g9), (12, 22, g12), (13, 20, g13)):
        f = _fmt(c, 1, False)
        for name, terms in _general_terms(f, c):
            out.append(_one("msm", c, f"marg c{c} {name}", terms, _lit(MARG, c, W, **g)))
    out.append(_one("msm", 12, "marg c12 second step", _second_step(_fmt(12, 1, False), 64, 2, 4), _lit(MARG, 12, 22, **g12)))
    out.append(_one("msm", 13, "marg c13 second step", _second_step(_fmt(13, 1, False), 64, 4, 4), _lit(MARG, 13, 20, **g13)))
    f16 = _fmt(16, 1, False)
    out.append(_one("msm", 16, "marg c16 equal", _terms(f16, p_equal(32767)), _lit(MARG, 16, 16, **g16)))
    out.append(_one("msm", 16, "marg c16 alt and single", _terms(f16, p_alt(32767)) + _terms(f16, p_rand(32767, 16), 3, fold_every=3) + _ends(f16, 7), _lit(MARG, 16, 16, **g16)))
    out.append(_one("msm", 16, "marg c16 second step", _second_step(f16, 256, 8, 16), _lit(MARG, 16, 16, **g16)))
    f15 = _fmt(15, 1, False)
    t15 = _terms(f15, p_rand(8191, 15)) + _terms(f15, p_equal(16383), 1) + _terms(f15, p_alt(16383), 2)
    out.append(_one("msm", 15, "marg c15 S1", t15, _lit(MARG, 15, 18, a=7, LO=128, HI=128, PR=64, PC=64, SR=2, SC=2, TR=8, TC=8), env=(("BPPP_MARG_S", "1"),)))
    out.append(_one("msm", 15, "marg c15 S64", t15, _lit(MARG, 15, 18, a=7, LO=128, HI=128, PR=2, PC=2, SR=64, SC=64, TR=8, TC=8), env=(("BPPP_MARG_S", "64"),)))
    # ---- batches.  Uniform widths; up to four instances are combined on the host, more in k_window_combine
    def batch(name, c, insts, want, per_instance=False, env=()):
        rows, logs = _pad([[s for s, _ in t] for t in insts], [[k for _, k in t] for t in insts])
        if not per_instance:                                        # shared points: one log list, the instances differ in their scalars alone
            assert all(l == logs[0] for l in logs), name
            logs = logs[0]
        out.append(Case(name, "batch", c, rows, logs, want, env))

    def shared(fmt, specs):
        """instances over ONE point list P_j = k_j G: instance i takes spec i's scalar where it has the log k_j, zero elsewhere"""
        pool = sorted({(s, b) for sp in specs for s, b in sp})
        return [[(s if (s, b) in set(sp) else 0, b) for s, b in pool] for sp in specs]
    f9b = _fmt(9, 3, False)
    gen9 = [t for _, t in _general_terms(f9b, 93)]
    batch("marg c9 batch 3 host combine", 9, shared(f9b, gen9[:3]), _lit(MARG, 9, 29, **g9))
    # k_window_combine with (W1, W2): r 2^(c-a) = +-W1 and (r 2^(c-a) + W1) 2^a = +-W2.  Bucket 0 gives W2 = b alone, bucket 16 (hi 1, lo 0) W1 = W2 = b
    comb9 = [_terms(f9b, {0: 1}, 20) + _terms(f9b, {16: 32}, 19), _terms(f9b, {0: 1}, 20) + _terms(f9b, {16: -32}, 19) + _terms(f9b, {3: 1}, 5),
             _terms(f9b, {0: 1}, 20) + _terms(f9b, {0: 512}, 19), _terms(f9b, {0: 1}, 20) + _terms(f9b, {0: -512}, 19) + _terms(f9b, {16: 5}, 4),
             _terms(f9b, {16: 1}, 20) + _terms(f9b, {0: 16}, 20)]
    batch("marg c9 batch 8 device combine", 9, shared(f9b, comb9 + gen9[:3]), _lit(MARG, 9, 29, combine=1, **dict(g9, PR=8, PC=8, SR=2, SC=2)))
    f8b = _fmt(8, 8, False)
    gen8 = [t for _, t in _general_terms(f8b, 83)]
    comb8 = [_terms(f8b, {0: 1}, 31) + _terms(f8b, {0: 256}, 30), _terms(f8b, {0: 1}, 31) + _terms(f8b, {0: -256}, 30) + _terms(f8b, {5: 1}, 3), _terms(f8b, {0: 1}, 0)]
    batch("wave c8 batch 8 device combine", 8, shared(f8b, comb8 + gen8), _lit(WAVE, 8, 32, combine=1, Lw=1, WPW=2))
    # ---- grouped route: thousands of windows
    def grouped(c, nbatch, seed, per_instance):
        f = _fmt(c, nbatch, False)
        gen = [t for _, t in _general_terms(f, seed)]
        rnd = random.Random(seed)
        few = lambda: [t for m in rnd.sample(range(f.M - 1), min(6, f.M - 1)) for t in _terms(f, {m: rnd.choice((1, -1, 2))}, rnd.choice((None, rnd.randrange(f.W - 1))))]
        insts = gen + [[], [t for t in gen[3]]] + [few() for _ in range(nbatch - len(gen) - 2)]       # one instance all zeros, one whose sum is 0 mod n
        if c == 2:
            insts = [_terms(f, {0: rnd.choice((1, -1, 2, 0))}) + _terms(f, {0: rnd.choice((1, -1))}, rnd.randrange(100)) + _ends(f, rnd.randrange(100), rnd.choice((1, -1)))
                     for _ in range(nbatch - 2)] + [[], _terms(f, {0: 1}) + _terms(f, {0: -1})]
        return insts if per_instance else shared(f, insts)
    batch("groups c2 batch 32", 2, grouped(2, 32, 20, False), _lit(GROUPS, 2, 128, combine=1, RG=2, Lw=1))
    batch("groups c5 batch 79", 5, grouped(5, 79, 50, True), _lit(GROUPS, 5, 52, combine=1, RG=8, Lw=2), per_instance=True)
    batch("groups c5 batch 79 RG1", 5, grouped(5, 79, 51, False), _lit(GROUPS, 5, 52, combine=1, RG=1, Lw=16), env=(("BPPP_RG", "1"),))
    batch("groups c5 batch 79 RG8", 5, grouped(5, 79, 52, False), _lit(GROUPS, 5, 52, combine=1, RG=8, Lw=2), env=(("BPPP_RG", "8"),))
    batch("groups c9 batch 142", 9, grouped(9, 142, 90, False), _lit(GROUPS, 9, 29, combine=1, RG=8, Lw=32))
    # ---- registered basis: one bucket set for all windows (the table holds 2^(c w) P_i), no window combine
    for c, want in ((8, _lit(WAVE, 8, 1, Lw=1, WPW=2)), (10, _lit(MARG, 10, 1, a=5, LO=32, HI=16, PR=32, PC=16, SR=1, SC=1, TR=1, TC=2))):
        ff = _fmt(c, 1, True)
        rnd = random.Random(c)
        below = [[(m + 1, b) for m, b in sorted(p.items()) if b] for p in (p_equal(ff.M - 1), p_alt(ff.M - 1), p_rand(ff.M - 1, c), P_ZERO_SUM, {}, p_rand(ff.M - 1, c + 1))]
        every = [(rnd.randrange(N), rnd.choice((1, -1, 2, -2, 0))) for _ in range(40)]                 # random scalars: digits in all windows
        for name, insts in (("batch 1 below", [below[2]]), ("batch 1 equal below", [below[0]]), ("batch 1 every window", [every]), ("batch 6", below[:5] + [every])):
            rows, logs = _pad([[s for s, _ in t] for t in shared(ff, insts)], [[k for _, k in t] for t in shared(ff, insts)])
            out.append(Case(f"basis c{c} {name}", "basis", c, rows, logs[0], dict(want, combine=int(len(insts) > 4))))
    assert len({x.name for x in out}) == len(out)
    return out


def _case(name):
    return next(x for x in cases() if x.name == name)


NAMES = [x.name for x in cases()]

# every loop of every replayed kernel, and the branches the case list must reach in it
LOOPS = ("r1.serial_run", "r1.serial_acc", "r1.scan", "r1.addacc", "r1.tree", "r2.scan", "r2.addacc", "r2.tree",
         "rg.serial_run", "rg.serial_acc", "rg.scan", "rg.addacc", "rg.tree", "marg.serial", "marg.tree",
         "tq.scan1", "tq.tree1", "tq.scan2", "tq.addA", "tq.tree2", "sm.scan", "sm.tree", "sm.addA", "sm.addT", "smj.serial", "smj.tree",
         "wc.add", "wc.add1", "wc.add2")
LADDERS = ("r1.ladder", "r2.ladder", "rg.ladder", "tq.dbl2", "sm.dbl64", "wc.dbl")
# (loop, branch) pairs no input reaches, each with the reason.  None is left: the scan and tree loops take all five branches on random small logs, the
# serial loops of k_reduce1 need BPPP_LW=2 and the one of k_msm_small_join 65 slices (BPPP_MSM_SMALL_LEN=64), and the second step of
# k_reduce_tail_quad, the two-wavefront lines of k_reduce2 and k_msm_small and the combines are reached by the constructed vectors above.
UNREACHABLE = {}


# ----------------------------------------------------------------------------- CPU-only tests
@pytest.mark.parametrize("c,balanced,want", [(6, True, (43, 41, 42)), (5, True, (52, 48, 51)), (7, True, (37, 34, 36)), (8, False, (32, 32, 31)), (2, False, (128, 128, 127)),
                                             (9, True, (29, 24, 28)), (9, False, (29, 29, -1)), (12, True, (22, 14, 21)), (13, True, (20, 16, 19)), (15, True, (18, 4, 17)),
                                             (16, False, (16, 16, 15)), (5, False, (52, 52, -1))])
def test_the_restated_format_round_trips(c, balanced, want):
    """window_layout pinned; every digit the inverse builds comes back from the forward recode in its window alone (or with the carry the
    extreme digit owes), through the sign fold too; random scalars over [0, n) decompose (Fmt.digits asserts sum e_w 2^off_w = +-v)"""
    assert _layout(c, balanced) == want
    f = Fmt(c, *want)
    rnd = random.Random(c)
    for s in [0, 1, N - 1, HALF, HALF + 1, HALF - 1] + [rnd.randrange(N) for _ in range(200)]:
        assert len(f.digits(s)) == f.W
    for w in sorted({0, 1, f.acnt - 1, min(f.acnt, f.W - 2), f.W - 2}):
        top = 1 << (f.cw[w] - 1)
        for d in sorted({1, 2, top - 1} - {0}):
            if d < top and d << f.off[w] <= HALF:
                e = f.digits(f.scalar(d, w))
                assert e[w] == d and sum(1 for x in e if x) == 1
                e = f.digits(N - f.scalar(d, w))
                assert e[w] == -d and sum(1 for x in e if x) == 1
        if w != f.top and w + 1 < f.W and (top << f.off[w]) <= HALF:
            e = f.digits(f.scalar(top, w))
            assert e[w] == -top and e[w + 1] == 1 and sum(1 for x in e if x) == 2
    if f.top >= 0:                                                  # the unbiased top row: digit 1 comes out positive after the negated store and the flip
        assert f.digits(1 << f.off[f.top])[f.top] == 1
        assert f.digits(HALF)[f.top] == 1 << (f.cw[f.top] - 1)      # and (n - 1) / 2 reaches its extreme bucket
    d = min(3, (1 << (min(f.cw) - 1)) - 1)
    e = f.digits(f.scalar(d))
    assert all(x in (0, d) for x in e) and sum(1 for x in e if x) >= f.W - 2


def test_the_plan_arithmetic_names_the_routes_the_cases_rely_on():
    for x in cases():
        env = dict(x.env)
        if x.kind == "small":
            rep, ln = _small_plan(x.n, int(env.get("BPPP_MSM_SMALL_C", 0)), int(env.get("BPPP_MSM_SMALL_LEN", 0)))
            assert ln == x.slice_len, x.name
        else:
            rep = _plan(x.c, x.batch, x.kind == "basis", int(env.get("BPPP_LW", 0)), int(env.get("BPPP_RG", 0)), int(env.get("BPPP_MARG_S", 0)))
        assert rep == x.want, (x.name, rep, x.want)
        if x.kind in ("msm", "batch"):
            assert x.n > 0 and (x.kind == "batch") == (x.batch > 1)
        if x.kind == "small":
            assert x.n <= 8192


@pytest.mark.parametrize("name", NAMES)
def test_the_replay_of_every_case_ends_in_its_reference(name):
    """the kernels' loops on integers reach (sum s_i k_i) mod n for every instance: the weighted-sum identities and the restated format hold"""
    x = _case(name)
    got, ev = x.replay()
    assert got == x.reference()
    assert sum(ev.values()) > 0


def test_the_cases_reach_every_branch_of_every_loop():
    total = collections.Counter()
    for x in cases():
        total.update(x.replay()[1])
    missing = [(l, b) for l in LOOPS for b in BRANCHES if not total[l, b] and (l, b) not in UNREACHABLE]
    assert not missing, missing
    assert not [k for k in UNREACHABLE if total[k]], "listed as unreachable, yet reached"
    for l in LADDERS:
        assert total[l, "dinf"] and total[l, "dpt"], l
    # quads of one wavefront on all three paths of xyzz_add_quad in the same scan step
    assert total["tq.scan1", "three paths in one step"] > 0
    assert not set(k[0] for k in total) - set(LOOPS) - set(LADDERS)


def test_the_patterns_have_the_effects_they_are_named_for():
    """on the marginal route: alternating signs cancel in every pair of lanes of the row trees (128 at c = 9), equal buckets double in the trees and
    in the first scan, the constructed vectors reach both same-x branches in every loop of the second step, a weighted sum of zero leaves infinity"""
    ev = _case("marg c9 alt").replay()[1]
    assert ev["marg.tree", "neg"] >= 128
    ev = _case("marg c9 equal").replay()[1]
    assert ev["tq.scan1", "dbl"] > 0 and ev["marg.tree", "dbl"] > 0
    ev = _case("marg c12 second step").replay()[1]
    assert all(ev[l, b] for l in ("tq.scan2", "tq.addA", "tq.tree2") for b in ("dbl", "neg"))
    got = _case("marg c9 zero").replay()[0]
    assert got == [None]
    ref = _case("groups c5 batch 79").reference()
    assert ref[3] is None and ref[5] is None and ref[6] is None and sum(1 for k in ref if k is None) == 3


# ----------------------------------------------------------------------------- the GPU side
def _pt_bytes(p):
    return bytes(64) if p is None else p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")


@pytest.fixture(scope="module")
def multiples(oracle_lib):
    """k -> k G as 64 result bytes, one oracle scalar multiplication each, kept for the module"""
    memo = {None: bytes(64), 0: bytes(64)}

    def get(k):
        if k not in memo:
            memo[k] = _pt_bytes(oracle_lib.mul(k % N, G))
        return memo[k]
    return get


@pytest.fixture(scope="module")
def contexts(gpu):
    """env -> context: the default one, and one per tuning the cases name, created under it (read once, at creation) with the environment restored"""
    import bulletproofspp_amd as b
    made = {(): gpu}
    for env in sorted({x.env for x in cases()} - {()}):
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env:
                mp.setenv(k, v)
            made[env] = b.Bppp(0)
    yield made
    for env, g in made.items():
        if env:
            g.close()


def _arr(blobs, width):
    return np.frombuffer(b"".join(blobs), dtype=np.uint64).reshape(-1, width).copy()


def _launch(g, x, multiples):
    sc = _arr([s.to_bytes(32, "little") for r in x.rows for s in r], 4)
    pts = _arr([multiples(k) for k in (x.logs if x.shared else [k for l in x.logs for k in l])], 8)
    if x.kind == "small":
        return [g.msm(sc, pts)]
    ds, dp = g.to_device(sc), g.to_device(pts)
    try:
        if x.kind == "msm":
            return [g.msm_device(ds, dp, x.n, window_bits=x.c)]
        if x.kind == "batch":
            return g.msm_batch_device(ds, dp, x.n, x.batch, shared_points=x.shared, window_bits=x.c)
        basis = g.basis(dp, window_bits=x.c, device=True, n=x.n)
        try:
            return basis.msm(ds, x.n, x.batch)
        finally:
            basis.close()
    finally:
        g.free(ds)
        g.free(dp)


def _report(g):
    from bulletproofspp_amd.capi import TestReduceReport, load_test_library
    rep = TestReduceReport()
    assert load_test_library().bppp_test_last_reduce(g.h, ctypes.byref(rep)) == 0
    return {n: getattr(rep, n) for n in FIELDS}


CROSS = ("small c6 rand", "marg c9 rand", "groups c2 batch 32")     # also compared with the oracle's innerProduct over the points


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_known_logs(contexts, multiples, oracle_lib, name):
    x = _case(name)
    g = contexts[x.env]
    got = _launch(g, x, multiples)
    assert _report(g) == x.want
    ref = x.reference()
    want = [multiples(k) for k in ref]
    if name in CROSS:
        pts = {k: oracle_lib.mul(k % N, G) if k % N else None for k in set(x.logs if x.shared else [k for l in x.logs for k in l])}
        for b in sorted({0, x.batch // 2, x.batch - 1}):
            assert _pt_bytes(oracle_lib.inner_product([(s, pts[k]) for s, k in zip(x.rows[b], x.logs_of(b))])) == want[b], (name, b)
    bad = [b for b in range(x.batch) if _pt_bytes(got[b]) != want[b]]
    assert not bad, f"{name}: {len(bad)} of {x.batch} instances differ from (sum s_i k_i) G, first {bad[:10]}"
    assert sum(1 for k in ref if k is None) == sum(1 for p in got if p is None)
