"""The bucket accumulation and the merges of csrc/msm.hip on points with KNOWN DISCRETE LOGS, the middle of the pipeline between the sort
(test_gpu_msm_sort_stage) and the bucket reductions (test_gpu_msm_reduce_known_logs, whose shape this file follows): k_acc_points, k_merge and
k_merge_heavy<false> (slices of L sorted entries per lane), k_order, k_acc_points_sized / k_acc_points_sized29 and k_merge_heavy<true> (whole
buckets by size), and k_msm_small's accumulation by result.

Every point is k_i G with a small signed k_i the test knows (0: the infinity point), or the lambda-image of such a point (the same y, x times
beta: log lambda k), so that what meets in an accumulator can be made equal, opposite or of equal y on purpose.  With hashed points the mixed
addition never sees its own accumulator again, and the merges add unrelated partial sums: the doubling and cancelling branches are not reached.

The unmarked tests replay the kernels lane for lane on integers (logs for points, None for infinity) over a given order of the sorted entries and
classify every operation:
  mixed additions (xyzz_madd, xyzz29_madd)   qinf / ainf: the point / the accumulator is infinity; gen; samey: R = 0 but Pd != 0, the two share their y
                                             only; dbl1, dblz, neg1, negz: P = Q, P = -Q, on an accumulator that holds one loaded point (ZZ = 1) or a sum
  xyzz_add, xyzz_add_chain                   rinf, linf, gen, dbl, neg, per loop (the classes of the reduce test)
and a few structural events (head / tail partials, the empty-bucket bisection, the shared_pts modes, whole buckets and pieces).  Each replay ends in
the plain reference: the sum of digit x log per bucket.  The union of the counts over the case list reaches every class of every loop but those in
UNREACHABLE.  On the CPU the order inside a (bucket, chunk) run is by term index; the GPU test reads the order the scatter produced back, replays
THAT, and requires the classes the case was built for (Case.must) again.  They are made certain by three constructions: a bucket filled from one
aligned group of 8 consecutive terms (one lane of any scatter places those in index order), the chunk contract (BPPP_HIST_CH: the runs of a
bucket follow the chunks), and multisets that end the same in every order ({A, B, -(A + B)}, all entries equal).

The GPU test asserts the route hooks and the layout against literals, then every bucket of every instance: its affine form is bit for bit (log) G
from a table of multiples built with the oracle, (0, 0) for log 0 and for an empty bucket; every stored sum keeps the magnitudes its readers accept (X <= 5, Y <= 3, ZZ and ZZZ <= 1), and on the
9 x 29-bit route every limb of a bucket that the accumulation kernel stores itself is below 2^26 (a bucket of several pieces is k_merge_heavy<true>'s
lazily reduced sum: xyzz_add_chain on 10 x 26-bit limbs)."""
import collections
import functools
import random

import numpy as np
import pytest

import msm_stages as S
import pyoracle as O
from test_gpu_msm_reduce_known_logs import _add, _fmt

N = O.N
G1 = (O.GX, O.GY)
LAM = (O.LAMBDA, O.LAMBDA * O.LAMBDA % N)
CAP, CHUNK, SERIAL_MAX = 128, 256, 8                                # ACC_CAP, HEAVY_CHUNK, MERGE_SERIAL_MAX of csrc/msm_plan.hpp
MADD = ("qinf", "ainf", "gen", "samey", "dbl1", "dblz", "neg1", "negz")
ADD = ("rinf", "linf", "gen", "dbl", "neg")


# ----------------------------------------------------------------------------- the replay
def _madd(ev, loop, acc, k):
    """acc += q as xyzz_madd / xyzz29_madd decide it.  acc: None (infinity) or (log, holds a sum); k: the log of q, None for the infinity point"""
    if k is None:
        ev[loop, "qinf"] += 1
        return acc
    if acc is None:
        ev[loop, "ainf"] += 1
        return (k, False)
    a, z = acc
    if a == k:
        ev[loop, "dblz" if z else "dbl1"] += 1
        return (2 * a % N, True)
    if a + k == N:
        ev[loop, "negz" if z else "neg1"] += 1
        return None
    ev[loop, "samey" if a in (k * LAM[0] % N, k * LAM[1] % N) else "gen"] += 1
    return ((a + k) % N, True)


def _log(acc):
    return None if acc is None else acc[0]


def _heavy(ev, name, parts):
    """k_merge_heavy for one bucket: per chunk of HEAVY_CHUNK partials the strided loop and the shuffle tree of one wavefront, then the last arriver's join"""
    def wave(loop, vals):
        acc = [None] * 64
        for lane in range(64):
            for t in range(lane, len(vals), 64):
                acc[lane] = _add(ev, name + "." + loop + "stride", acc[lane], vals[t])
        d = 32
        while d >= 1:
            acc = [_add(ev, name + "." + loop + "tree", acc[l], acc[l + d]) if l + d < 64 else acc[l] for l in range(64)]
            d >>= 1
        return acc[0]
    sums = [wave("", parts[t0:t0 + CHUNK]) for t0 in range(0, len(parts), CHUNK)]
    ev[name, "one chunk" if len(sums) == 1 else "join"] += 1
    return sums[0] if len(sums) == 1 else wave("join_", sums)


def _entry_log(plog, e, pidx_of):
    k = plog[pidx_of(e & 0x7FFFFFFF)]
    return k if k is None or not e >> 31 else N - k


def replay_slices(P, start, count, order, plog):
    """k_acc_points, k_merge, k_merge_heavy<false>.  P: FB, L, G, n, WM, shared; returns ({bucket: log or None}, events)"""
    ev = collections.Counter()
    FB, L, n, WM, shared = P["FB"], P["L"], P["n"], P["WM"], P["shared"]
    total = start[FB]
    buckets, rec = {}, {}
    assert -(-total // L) <= P["G"]
    ev["acc.shared", shared if shared < 2 else "d"] += 1
    for g in range(-(-total // L)):                                 # the lanes past the entries return at once
        pos0, pos1 = g * L, min(total, g * L + L)
        lo, hi = 0, FB - 1
        while lo < hi:
            mid = lo + (hi - lo + 1) // 2
            if start[mid] <= pos0:
                lo = mid
            else:
                hi = mid - 1
        cur, end = lo, start[lo + 1]
        from_prev, first, acc = start[cur] < pos0, True, None
        for p in range(pos0, pos1):
            if p == end:
                if first and from_prev:
                    rec[2 * g] = acc; ev["acc.store", "head"] += 1
                else:
                    buckets[cur] = acc; ev["acc.store", "bucket"] += 1
                first, acc = False, None
                cur += 1
                end = start[cur + 1]
                if end <= p:                                        # empty buckets: bisect for the one that holds p
                    ev["acc.bisect", "taken"] += 1
                    lo2, hi2 = cur + 1, FB - 1
                    while lo2 < hi2:
                        mid = lo2 + (hi2 - lo2 + 1) // 2
                        if start[mid] <= p:
                            lo2 = mid
                        else:
                            hi2 = mid - 1
                    cur, end = lo2, start[lo2 + 1]
                else:
                    ev["acc.bisect", "next"] += 1
            inst = cur // WM
            acc = _madd(ev, "acc.madd", acc, _entry_log(plog, order[p], (lambda i: i) if shared == 1 else (lambda i: (inst // (shared or 1)) * n + i)))
        if first and from_prev:
            rec[2 * g] = acc; ev["acc.store", "head and on" if end > pos1 else "head"] += 1
        elif end > pos1:
            rec[2 * g + 1] = acc; ev["acc.store", "tail"] += 1
        else:
            buckets[cur] = acc; ev["acc.store", "bucket"] += 1
    for fb in np.flatnonzero(count).tolist():
        s, cnt = start[fb], int(count[fb])
        g0, g1 = s // L, (s + cnt - 1) // L
        if g0 == g1:
            ev["merge", "one lane"] += 1
            continue
        parts = [_log(rec[2 * g0 + 1])] + [_log(rec[2 * (g0 + t)]) for t in range(1, g1 - g0 + 1)]
        if len(parts) > SERIAL_MAX + 1:
            buckets[fb] = (_heavy(ev, "heavy", parts),)
            continue
        ev["merge", "serial"] += 1
        acc = parts[0]
        for p in parts[1:]:
            acc = _add(ev, "merge.serial", acc, p)
        buckets[fb] = (acc,)
    ev["merge", "empty"] += FB - int(np.count_nonzero(count))
    return {fb: _log(a) for fb, a in buckets.items()}, ev


def replay_sized(P, start, count, order, plog):
    """k_order (items by size class, pieces of ACC_CAP, piece_base in bucket order: any order gives the same sums), acc_points_sized, k_merge_heavy<true>"""
    ev = collections.Counter()
    classes = [[] for _ in range(CAP + 1)]
    piece_base, slots = {}, 0
    for fb in np.flatnonzero(count).tolist():
        cnt = int(count[fb])
        full, rem = divmod(cnt, CAP)
        classes[CAP] += [(fb, j) for j in range(full)]
        if rem:
            classes[rem].append((fb, full))
        if cnt > CAP:
            piece_base[fb] = slots
            slots += full + (1 if rem else 0)
            ev["order", "pieces, the last short" if rem else "pieces, all full"] += 1
        else:
            ev["order", "whole"] += 1
    items = [it for size in range(CAP, 0, -1) for it in classes[size]]
    assert len(items) <= P["items_max"] and 2 * (P["total_max"] // CAP) + 2 >= slots
    buckets, pieces, seen = {}, {}, 0
    for fb, pc in items:
        cnt, first = int(count[fb]), pc * CAP
        ln = min(CAP, cnt - first)
        assert ln >= 1
        ent = order[start[fb] + first:start[fb] + first + ln]
        seen += ln
        k = _entry_log(plog, ent[0], lambda i: i)
        ev["sized.load", "inf" if k is None else "pt"] += 1
        acc = None if k is None else (k, False)
        for e in ent[1:]:
            acc = _madd(ev, "sized.madd", acc, _entry_log(plog, e, lambda i: i))
        if cnt > CAP:
            pieces[piece_base[fb] + pc] = _log(acc)
        else:
            buckets[fb] = _log(acc)
    assert seen == start[P["FB"]] and len(pieces) == slots
    for fb, base in piece_base.items():
        buckets[fb] = _heavy(ev, "sheavy", [pieces[base + t] for t in range(-(-int(count[fb]) // CAP))])
    return buckets, ev


# ----------------------------------------------------------------------------- the plan arithmetic, restated
def _plan(kind, c, n, batch, env):
    """plan_windows, the forced chunk count and plan_accumulate of csrc/msm_plan.hpp"""
    flat = kind == "basis"
    fmt = _fmt(c, batch, flat)
    M, NB = fmt.M, batch * fmt.W
    total_max = NB * n
    FB = (batch if flat else NB) * M
    env = dict(env)
    if batch == 1 and not flat:
        occ, lo, L = n // M, 8, 64
        while lo < 64 and 4 * lo < occ:
            lo <<= 1
        while L > lo and total_max // L < 150000:
            L >>= 1
    else:
        L = 4
        while L < 64 and total_max // (2 * L) >= 65536:
            L <<= 1
        if flat:
            while L < 128 and total_max / FB > 4.0 * L and total_max // (2 * L) >= 65536:
                L <<= 1
    if "BPPP_LACC" in env:
        L = int(env["BPPP_LACC"])
    CH = int(env["BPPP_HIST_CH"])
    sized = batch == 1 and not flat and (int(env.get("BPPP_ACC_SIZED", -1)) > 0 or ("BPPP_ACC_SIZED" not in env and c == 16))
    return dict(W=fmt.W, CH=CH, per=(-(-n // CH) + 7) & ~7, L=L, G=-(-total_max // L) or 1, sized=int(sized), fq29=int(sized and env.get("BPPP_ACC_FQ29", "1") != "0"))


# ----------------------------------------------------------------------------- cases
class Build:
    """terms of one scalar row, by chunk: chunk k of CH occupies the term indices [k per, (k + 1) per) with n = CH per - 1, so that (n / CH rounded up,
    then to 8) = per.  A term is (the buckets (window, |digit|) it enters - one scalar may have a digit in several windows -, the log of its point, fold:
    the same entry through the sign fold, as (n - s, -k G))"""

    def __init__(self, fmt, CH=1, per=0):
        self.fmt, self.CH, self.per, self.chunks = fmt, CH, per, [[] for _ in range(CH)]
        self.w, self.d = 0, 0

    def fresh(self):
        """the next unused bucket, in the windows of full width below the top"""
        self.d += 1
        if self.d >= min(self.fmt.M, 1 << (self.fmt.cw[self.w] - 1)):
            self.w, self.d = self.w + 1, 1
        assert self.w < min(self.fmt.acnt, self.fmt.W - 1) - 8
        return (self.w, self.d)

    def wide(self, count):
        """`count` buckets in as many windows, the highest full-width ones below the top: one scalar can enter them all"""
        assert count <= 8
        top = min(self.fmt.acnt, self.fmt.W - 1) - 1
        return [(top - i, 1 + i) for i in range(count)]

    def term(self, chunk, buckets, k, fold=False):
        """buckets: (window, |digit|) or (window, |digit|, -1) for a negative digit (below a positive one in a higher window)"""
        s = sum((b[2] if len(b) > 2 else 1) * self.fmt.scalar(b[1], b[0]) for b in buckets)
        assert 0 < s <= (N - 1) // 2
        self.chunks[chunk].append((N - s, -k) if fold else (s, k))

    def group(self, chunk, bucket, entries):
        """one aligned group of 8 consecutive terms: the entries (log, fold) of one bucket in index order, placed by one lane"""
        assert 0 < len(entries) <= 8
        lst = self.chunks[chunk]
        lst += [(0, 1)] * (-len(lst) % 8)
        for k, fold in entries:
            self.term(chunk, [bucket], k, fold)
        lst += [(0, 1)] * (-len(lst) % 8)

    def fill(self, chunk, buckets, k, count, fold=False):
        for _ in range(count):
            self.term(chunk, buckets, k, fold)

    def finish(self):
        per = max([self.per] + [(len(l) + (8 if k == self.CH - 1 else 7)) & ~7 for k, l in enumerate(self.chunks)])
        n = self.CH * per - 1
        terms = []
        for k, l in enumerate(self.chunks):
            terms += l + [(0, 1)] * ((per if k < self.CH - 1 else per - 1) - len(l))
        assert len(terms) == n
        return [s for s, _ in terms], [k for _, k in terms], per


def E(**kw):
    return tuple(sorted((k, str(v)) for k, v in kw.items()))


class Case:
    """kind: 'msm' (bppp_msm_device with window_bits), 'batch' (bppp_msm_batch_device), 'basis' (Basis.msm).  rows [batch][n] scalars; logs: n for shared
    points (shared = 1), batch n for points per instance (0), (batch / 2) n for points per pair of instances (2).  want: the literal the layout and
    the spans must show; must: the (loop, class) pairs the case was built for, required of the order the GPU produced too"""

    def __init__(self, name, kind, c, env, rows, logs, shared, want, must):
        self.name, self.kind, self.c, self.env, self.rows, self.logs, self.shared, self.want, self.must = name, kind, c, env, rows, logs, shared, want, must
        self.batch, self.n, self.flat = len(rows), len(rows[0]), kind == "basis"
        assert len(logs) == self.n * (1 if shared == 1 else self.batch if shared == 0 else self.batch // 2)

    @functools.lru_cache(maxsize=None)
    def prepared(self):
        """the sort's output by the restated format (msm_stages), in the canonical order: runs by chunk, a run by term index"""
        fmt = _fmt(self.c, self.batch, self.flat)
        plan = _plan(self.kind, self.c, self.n, self.batch, self.env)
        stored, neg = S.recode(fmt, self.rows)
        ts = self.n if self.flat else 0
        fb, run, ent = S.entries(fmt, stored, neg, self.flat, plan["CH"], plan["per"], ts)
        o = np.lexsort((ent & 0x7FFFFFFF, run, fb))
        FB = (self.batch if self.flat else self.batch * fmt.W) * fmt.M
        count = np.bincount(fb, minlength=FB)
        start = [0] + np.cumsum(count).tolist()
        if self.flat:                                               # the table: row w holds 2^(c w) P_j
            plog = [(k << (self.c * w)) % N or None for w in range(fmt.W) for k in self.logs]
        else:
            plog = [k % N or None for k in self.logs]
        P = dict(plan, FB=FB, n=self.n, WM=(1 if self.flat else fmt.W) * fmt.M, shared=self.shared, total_max=self.batch * fmt.W * self.n)
        P["items_max"] = min(P["total_max"], FB + P["total_max"] // CAP)
        # the reference: sum of digit x log per bucket
        ref = collections.defaultdict(int)
        for f, e in zip(fb.tolist(), ent.tolist()):
            inst = f // P["WM"]
            k = plog[(e & 0x7FFFFFFF) if self.shared == 1 else (inst // (self.shared or 1)) * self.n + (e & 0x7FFFFFFF)]
            if k is not None:
                ref[f] += -k if e >> 31 else k
        ref = {f: v % N or None for f, v in ref.items()}
        return fmt, P, count, start, ent[o].tolist(), plog, ref

    def replay(self, order=None):
        fmt, P, count, start, canon, plog, ref = self.prepared()
        got, ev = (replay_sized if P["sized"] else replay_slices)(P, start, count, canon if order is None else order, plog)
        assert set(got) == set(np.flatnonzero(count).tolist())
        assert all(got[f] == ref.get(f) for f in got), [f for f in got if got[f] != ref.get(f)][:5]
        return got, ev

    def spans(self):
        """the literal's view of the buckets: entries in all, the largest bucket, the most partial sums (lanes or pieces) one bucket has"""
        fmt, P, count, start, *_ = self.prepared()
        nz = np.flatnonzero(count)
        if P["sized"]:
            np_ = -(-count[nz] // CAP)
        else:
            st = np.array(start[:-1])[nz]
            np_ = (st + count[nz] - 1) // P["L"] - st // P["L"] + 1
        return dict(total=start[-1], cnt_max=int(count.max()), np_max=int(np_.max()))


def _lam(k, t=1):
    return k * LAM[t - 1] % N


def _patterns(rnd, chunked):
    """directed buckets: (entries of chunk 0, entries of chunk 1), an entry (log, fold); chunked: also the ones that rely on the chunk contract"""
    pick = lambda *avoid: next(k for k in iter(lambda: rnd.choice((1, -1)) * rnd.randrange(1, 40), None) if k not in avoid)
    a = pick(); b = pick(a, -a); d = pick(a + b, -(a + b), 2 * (a + b), -2 * (a + b)); s = a + b
    f = lambda *ks: [(k, rnd.random() < 0.3) for k in ks]            # some entries through the sign fold
    seven = [pick() for _ in range(7)]
    while not sum(seven) or any(not sum(seven[:j]) for j in range(2, 7)):
        seven = [pick() for _ in range(7)]
    out = [(f(a, a), []), (f(a, -a), []), (f(a, b, s), []), (f(a, b, -s), []), (f(a, b, s, d), []), (f(a, b, -s, d), []), (f(a, -a, b), []), (f(0, a), []),
           (f(a, 0, b), []), (f(a, 0), []), (f(0, 0), []), (f(a, _lam(a)), []), (f(a, b, _lam(s)), []), (f(a, b, _lam(s, 2), d), []), (f(a), []),
           (f(*[a] * 8), []), (f(*[a, -a] * 4), []), (f(*seven, sum(seven)), []), (f(*seven, -sum(seven)), []), (f(a, a, 2 * a, 4 * a, -8 * a, d), [])]
    if chunked:
        out += [(f(a, b), f(s)), (f(a, b), f(-s)), (f(a), f(a)), (f(a), f(-a)), (f(a, b), f(_lam(s))), (f(a, b, d), f(-s - d, a)), (f(a, -a), f(b, b)), (f(0), f(a))]
    return out


def _directed(fmt, CH, seed, reps=4, extra=None):
    """reps sets of the directed buckets, each bucket from one aligned group per chunk; extra(build): further terms, in buckets before those"""
    rnd = random.Random(seed)
    bd = Build(fmt, CH)
    if extra:
        extra(bd)
    for _ in range(reps):
        for e0, e1 in _patterns(rnd, CH > 1):
            bucket = bd.fresh()
            bd.group(0, bucket, e0)
            if e1:
                bd.group(CH - 1, bucket, e1)
    return bd


M_ACC = {("acc.madd", x) for x in MADD}
M_SIZED = {("sized.madd", x) for x in MADD}
M_SERIAL = {("merge.serial", x) for x in ("gen", "dbl", "neg")}


def _one(name, kind, c, env, bd, want, must):
    row, logs, _ = bd.finish()
    return Case(name, kind, c, env, [row], logs, 1, want, must)


def _heavy_slices(bd):
    """L = 4; these buckets come first, so the first one starts at position 0 and those after a multiple of 4 entries start on a lane's border.  More than 256
    partial sums, so several chunks and the join: 2048 equal entries (512 partials: equal chunk sums), 1024 and then, from the second chunk of the sort, 1024
    opposite ones, 1020 and then 44 at infinity (the second chunk sum is infinity wherever the bucket starts), 1024 at infinity and then 40.  More than 9 in one
    chunk: 128 + 128 opposite (the tree cancels), 256 and then 64 opposite (lane t of the strided loop adds partial 64 + t to partial t: cancels), 128 at
    infinity and then 128 (linf in the tree), 40 at infinity, 300 equal ones (75 or 76 partials: lanes 0 .. 11 double), 1100 equal ones, and short spans"""
    for k0, n0, k1, n1 in ((1, 2048, 0, 0), (1, 1024, -1, 1024), (3, 1020, 0, 44), (0, 1024, 1, 40), (2, 128, -2, 128), (1, 256, -1, 64), (0, 128, 1, 128), (0, 40, 0, 0),
                           (1, 300, 0, 0), (1, 1100, 0, 0), (1, 37, 0, 0), (1, 36, -1, 36), (2, 20, 2, 16)):
        bucket = bd.fresh()
        bd.fill(0, [bucket], k0, n0)
        if n1:
            bd.fill(bd.CH - 1, [bucket], k1, n1)


def _sized_sizes(bd):
    """whole buckets and pieces: 1, 2, 127, 128, 129 and 257 equal entries, 129 and 257 whose last piece is opposite to the sum of the others (second chunk of
    the sort), two full pieces of points at infinity, a piece at infinity before a full one (linf in the tree), opposite, equal and unequal pieces"""
    for k0, n0, k1, n1 in ((1, 1, 0, 0), (1, 2, 0, 0), (1, 127, 0, 0), (1, 128, 0, 0), (1, 129, 0, 0), (1, 257, 0, 0), (1, 128, -128, 1), (1, 256, -256, 1), (0, 256, 0, 0),
                           (0, 128, 1, 128), (1, 128, -1, 128), (2, 128, 2, 128), (1, 128, 3, 100)):
        bucket = bd.fresh()
        bd.fill(0, [bucket], k0, n0)
        if n1:
            bd.fill(bd.CH - 1, [bucket], k1, n1)


def _sized_stride(bd):
    """more than 64 pieces: 8192 terms with a digit in four windows, then in the second chunk of the sort 128 equal entries (lane 0 of the strided loop doubles),
    128 opposite ones (cancels), 100 (general) and 128 at infinity, one window each"""
    bs = bd.wide(4)
    bd.fill(0, bs, 1, 64 * CAP)
    for bucket, k, cnt in zip(bs, (1, -1, 1, 0), (CAP, CAP, 100, CAP)):
        bd.fill(bd.CH - 1, [bucket], k, cnt)


def _sized_join(bd):
    """more than 256 pieces: 32768 terms (chunks 0 .. 7 of 9 of the sort, 4096 terms each) of G with a digit in five windows: 256 full pieces, one chunk of
    partial sums.  The last chunk of the sort brings the second chunk of partial sums, one window each: 128 entries of 256 G (equal chunk sums: the join doubles),
    of -256 G (cancels), 100 of 5 G (general), 128 at infinity (rinf).  In the fifth window the digit is negative in chunks 4 .. 7 of the sort: pieces 0 .. 127 are
    128 G, pieces 128 .. 255 the opposite, every lane of the strided loop ends in infinity and so does the first chunk sum (linf in the join)"""
    bs = bd.wide(5)
    for ch in range(8):
        bd.fill(ch, bs[:4] + [bs[4] + ((1 if ch < 4 else -1),)], 1, 4096)
    for bucket, k, cnt in zip(bs, (256, -256, 5, 0, 7), (CAP, CAP, 100, CAP, 100)):
        bd.fill(8, [bucket], k, cnt)


def _l1_join(bd):
    """L = 1: every entry a partial sum.  16384 terms with a digit in four windows (64 chunks of 256 partial sums), then from the second chunk of the sort a
    65th chunk that lane 0 of the join adds to the first: 256 entries of G (doubles), of -G (cancels), of 2 G (general), at infinity (rinf)"""
    bs = bd.wide(4)
    bd.fill(0, bs, 1, 64 * CHUNK)
    for bucket, k in zip(bs, (1, -1, 2, 0)):
        bd.fill(1, [bucket], k, CHUNK)


def _variants(row, batch):
    """the instances of a batch over the scalars of one row: whole groups of 8 terms negated (the patterns keep their shape) or left out"""
    return [[0 if (j // 8 + 2 * b) % 5 == 4 else (N - s) % N if (j // 8 + b) % 3 == 2 else s for j, s in enumerate(row)] for b in range(batch)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    H = lambda name: {(name + "." + loop, x) for loop in ("stride", "tree") for x in ("gen", "dbl", "neg")}
    J = lambda name: {(name + ".join_tree", x) for x in ("gen", "dbl", "neg")} | {(name + ".join_stride", "rinf")}
    # ---- slices: one MSM with explicit window_bits
    f5, f9, f13, f16 = (_fmt(c, 1, False) for c in (5, 9, 13, 16))
    out.append(_one("slices c5 directed", "msm", 5, E(BPPP_LACC=4, BPPP_HIST_CH=1), _directed(f5, 1, 5),
                    dict(W=52, CH=1, per=648, L=4, G=8411, sized=0, fq29=0, total=312, cnt_max=8, np_max=3), M_ACC | M_SERIAL))
    out.append(_one("slices c9 directed, the plan's L, two chunks", "msm", 9, E(BPPP_HIST_CH=2), _directed(f9, 2, 9),
                    dict(W=29, CH=2, per=896, L=8, G=6493, sized=0, fq29=0, total=408, cnt_max=8, np_max=2), M_ACC | {("merge.serial", "dbl"), ("merge.serial", "neg")}))
    out.append(_one("slices c13 directed, two chunks", "msm", 13, E(BPPP_LACC=4, BPPP_HIST_CH=2), _directed(f13, 2, 13),
                    dict(W=20, CH=2, per=896, L=4, G=8955, sized=0, fq29=0, total=408, cnt_max=8, np_max=3), M_ACC | M_SERIAL))
    out.append(_one("slices c5 heavy", "msm", 5, E(BPPP_LACC=4, BPPP_HIST_CH=2), _directed(f5, 2, 55, reps=1, extra=_heavy_slices),
                    dict(W=52, CH=2, per=7392, L=4, G=192179, sized=0, fq29=0, total=8743, cnt_max=2048, np_max=512), H("heavy") | J("heavy") | M_SERIAL))
    out.append(_one("slices c13 L1 join", "msm", 13, E(BPPP_LACC=1, BPPP_HIST_CH=2), _directed(f13, 2, 131, reps=1, extra=_l1_join),
                    dict(W=20, CH=2, per=16608, L=1, G=664300, sized=0, fq29=0, total=66662, cnt_max=16640, np_max=16640),
                    {("heavy.join_stride", x) for x in ("gen", "dbl", "neg", "rinf", "linf")}))
    # ---- whole buckets by size, on 10 x 26 and on 9 x 29 limbs
    for c, fmt in ((5, f5), (13, f13), (16, f16)):
        for fq29 in (0, 1):
            env = E(BPPP_ACC_SIZED=1, BPPP_ACC_FQ29=fq29, BPPP_HIST_CH=2)
            tag = f"sized {'9 x 29' if fq29 else '10 x 26'} c{c}"
            want = dict(W={5: 52, 13: 20, 16: 16}[c], CH=2, per=2248, L={5: 64, 13: 8, 16: 8}[c], G={5: 3653, 13: 11238, 16: 8990}[c], sized=1, fq29=fq29, total=2486, cnt_max=257, np_max=3)
            out.append(_one(tag + " directed and sizes", "msm", c, env, _directed(fmt, 2, 100 + c, reps=2, extra=_sized_sizes), want,
                            M_SIZED | {("sheavy.tree", x) for x in ("gen", "dbl", "neg", "rinf")} | {("sized.load", "inf"), ("order", "whole"), ("order", "pieces, all full"),
                                                                                                         ("order", "pieces, the last short")}))
    for c, fmt, fq29 in ((5, f5, 0), (16, f16, 1)):
        env = E(BPPP_ACC_SIZED=1, BPPP_ACC_FQ29=fq29, BPPP_HIST_CH=2)
        out.append(_one(f"sized {'9 x 29' if fq29 else '10 x 26'} c{c} more than 64 pieces", "msm", c, env, _directed(fmt, 2, 200 + c, reps=1, extra=_sized_stride),
                        dict(W={5: 52, 16: 16}[c], CH=2, per=8416, L={5: 64, 16: 8}[c], G={5: 13676, 16: 33662}[c], sized=1, fq29=fq29, total=33354, cnt_max=8320, np_max=65),
                        {("sheavy.stride", x) for x in ADD} | {("sheavy", "one chunk")}))
    for c, fmt, fq29 in ((13, f13, 0), (16, f16, 1)):
        env = E(BPPP_ACC_SIZED=1, BPPP_ACC_FQ29=fq29, BPPP_HIST_CH=9)
        out.append(_one(f"sized {'9 x 29' if fq29 else '10 x 26'} c{c} join", "msm", c, env, _directed(fmt, 9, 300 + c, reps=0, extra=_sized_join),
                        dict(W={13: 20, 16: 16}[c], CH=9, per=4096, L=8, G={13: 92158, 16: 73726}[c], sized=1, fq29=fq29, total=164424, cnt_max=32896, np_max=257),
                        J("sheavy") | {("sheavy", "join")}))
    # ---- batches (uniform widths) and a registered basis: slices
    bd = _directed(_fmt(5, 3, False), 1, 35)
    row, logs, per = bd.finish()
    out.append(Case("batch 3 shared c5", "batch", 5, E(BPPP_HIST_CH=1), _variants(row, 3), logs, 1,
                    dict(W=52, CH=1, per=648, L=4, G=25233, sized=0, fq29=0, total=756, cnt_max=8, np_max=3), M_ACC | {("acc.shared", 1)}))
    bd = _directed(_fmt(8, 5, False), 2, 85)
    row, logs, per = bd.finish()
    out.append(Case("batch 5 per instance c8, two chunks", "batch", 8, E(BPPP_HIST_CH=2), _variants(row, 5), [k * (b + 1) for b in range(5) for k in logs], 0,
                    dict(W=32, CH=2, per=896, L=4, G=71640, sized=0, fq29=0, total=1632, cnt_max=8, np_max=3), M_ACC | {("acc.shared", 0)}))
    out.append(Case("batch 4 in pairs c8, two chunks", "batch", 8, E(BPPP_HIST_CH=2), _variants(row, 4), [k * (p + 2) for p in range(2) for k in logs], 2,
                    dict(W=32, CH=2, per=896, L=4, G=57312, sized=0, fq29=0, total=1309, cnt_max=8, np_max=3), M_ACC | {("acc.shared", "d")}))
    # a registered basis: one bucket set for all windows, the runs of a bucket in (window, chunk) order; the point of window w is 2^(8 w) P
    ff = _fmt(8, 1, True)
    bd = _directed(ff, 1, 8)
    rnd = random.Random(88)
    for _ in range(6):                                              # a pair, or a sum, from window 0 meets its like from window 1
        a, b = rnd.randrange(1, 30), rnd.randrange(31, 60)
        for lo, hi in (([(256 * a, False)], [(a, False)]), ([(256 * a, False)], [(-a, False)]), ([(256 * a, False), (256 * b, False)], [(a + b, False)]),
                       ([(256 * a, False), (256 * b, True)], [(-a - b, True)])):
            bd.d += 1
            assert bd.d < 127
            bd.group(0, (0, bd.d), lo)
            bd.group(0, (1, bd.d), hi)
    out.append(_one("basis c8", "basis", 8, E(BPPP_HIST_CH=1), bd,
                    dict(W=33, CH=1, per=1032, L=4, G=8506, sized=0, fq29=0, total=372, cnt_max=8, np_max=3), M_ACC | {("acc.shared", 1)}))
    assert len({x.name for x in out}) == len(out)
    return out


def _case(name):
    return next(x for x in cases() if x.name == name)


NAMES = [x.name for x in cases()]
LOOPS_MADD = ("acc.madd", "sized.madd")
LOOPS_ADD = ("merge.serial", "heavy.stride", "heavy.tree", "heavy.join_stride", "heavy.join_tree", "sheavy.stride", "sheavy.tree", "sheavy.join_stride", "sheavy.join_tree")
STRUCT = [("acc.store", x) for x in ("head", "head and on", "tail", "bucket")] + [("acc.bisect", "taken"), ("acc.bisect", "next"), ("acc.shared", 1), ("acc.shared", 0),
          ("acc.shared", "d"), ("merge", "one lane"), ("merge", "serial"), ("merge", "empty"), ("heavy", "one chunk"), ("heavy", "join"), ("sheavy", "one chunk"), ("sheavy", "join"),
          ("order", "whole"), ("order", "pieces, all full"), ("order", "pieces, the last short"), ("sized.load", "inf"), ("sized.load", "pt")]
# (loop, class) pairs no case reaches, with the reason
UNREACHABLE = {
    # lane j of the join adds chunk sums j, j + 64, ...: a second one needs 65 chunks of 256 pieces of 128 entries, 2^21 entries in ONE bucket.  The same loop of
    # k_merge_heavy<false> is reached with 16 640 entries at L = 1 ("slices c13 L1 join"); the template shares the code.
    ("sheavy.join_stride", "gen"): "more than 2^21 entries in one bucket", ("sheavy.join_stride", "dbl"): "more than 2^21 entries in one bucket",
    ("sheavy.join_stride", "neg"): "more than 2^21 entries in one bucket",
}


# ----------------------------------------------------------------------------- CPU-only tests
@pytest.mark.parametrize("name", NAMES)
def test_the_replay_of_every_case_ends_in_its_reference(name):
    """the kernels' loops on integers reach the sum of digit x log of every bucket (Case.replay asserts it), on the canonical order and on one with every run
    reversed; the plan figures and the spans the case relies on are the literals; the classes the case was built for are reached"""
    x = _case(name)
    fmt, P, count, start, canon, plog, ref = x.prepared()
    got, ev = x.replay()
    fb, run, ent = S.observed_runs(np.array(canon, dtype=np.uint32), count, x.flat, P["CH"], P["per"], x.n if x.flat else 0)
    assert x.replay(ent[np.lexsort((-(ent & 0x7FFFFFFF), run, fb))].tolist())[0] == got
    assert {k: P[k] for k in ("W", "CH", "per", "L", "G", "sized", "fq29")} | x.spans() == x.want, ({k: P[k] for k in ("per", "L", "G")}, x.spans())
    assert x.n <= 40000 and x.n % 2 == 1
    assert not x.must - set(k for k in ev if ev[k]), sorted(x.must - set(ev), key=str)
    assert any(v is None for v in got.values()) and any(v is not None for v in got.values())


def test_the_cases_reach_every_class_of_every_loop():
    total = collections.Counter()
    for x in cases():
        total.update(x.replay()[1])
    want = [(l, b) for l in LOOPS_MADD for b in MADD] + [(l, b) for l in LOOPS_ADD for b in ADD] + STRUCT
    missing = [k for k in want if not total[k] and k not in UNREACHABLE]
    assert not missing, missing
    assert not [k for k in UNREACHABLE if total[k]], "listed as unreachable, yet reached"
    assert not set(total) - set(want), set(total) - set(want)


def test_the_replay_follows_the_order_it_is_given():
    """[A, B, A + B] doubles on a sum; with A + B first the same multiset takes two general additions: the classes are those of the order, not of the case"""
    ev = collections.Counter()
    acc = None
    for k in (3, 4, 7):
        acc = _madd(ev, "x", acc, k)
    assert acc == (14, True) and ev["x", "dblz"] == 1 and ev["x", "gen"] == 1
    ev = collections.Counter()
    acc = None
    for k in (7, 3, 4):
        acc = _madd(ev, "x", acc, k)
    assert acc == (14, True) and ev["x", "gen"] == 2 and not ev["x", "dblz"]
    acc = _madd(ev, "x", (5, False), _lam(5))
    assert ev["x", "samey"] == 1 and acc == ((5 + _lam(5)) % N, True) and (1 + LAM[0] + LAM[1]) % N == 0
    assert _madd(ev, "x", (5, True), N - 5) is None and ev["x", "negz"] == 1


# ----------------------------------------------------------------------------- the GPU side
@pytest.fixture(scope="module")
def contexts(gpu):
    made = S.make_contexts(gpu, [x.env for x in cases()])
    yield made
    S.close_contexts(made)


@pytest.fixture(scope="module")
def multiples(oracle_lib):
    """log -> (log) G as the 16 words of an affine bucket ((0, 0) for None), one oracle scalar multiplication each"""
    memo = {None: np.zeros(16, dtype=np.uint32)}

    def get(k):
        if k not in memo:
            x, y = oracle_lib.mul(k % N, G1)
            memo[k] = np.frombuffer(x.to_bytes(32, "little") + y.to_bytes(32, "little"), dtype=np.uint32)
        return memo[k]
    assert oracle_lib.mul(O.LAMBDA, G1) == (O.BETA * O.GX % O.P, O.GY)
    return get


def _launch(g, x, multiples):
    sc = np.frombuffer(b"".join(s.to_bytes(32, "little") for r in x.rows for s in r), dtype=np.uint64).reshape(-1, 4).copy()
    pts = np.stack([multiples(k % N or None) for k in x.logs]).view(np.uint64).reshape(-1, 8).copy()
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
        g.free(ds); g.free(dp)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_known_logs(contexts, multiples, name):
    x = _case(name)
    g = contexts[x.env]
    fmt, P, count, start, canon, plog, ref = x.prepared()
    got_pts = _launch(g, x, multiples)
    lay = S.layout(g)
    assert S.hooks(g)[2:] == (x.want["sized"], x.want["fq29"])
    assert {k: lay[k] for k in ("W", "CH", "per", "L", "G", "sized", "fq29", "total")} == {k: x.want[k] for k in ("W", "CH", "per", "L", "G", "sized", "fq29", "total")}
    assert (lay["c"], lay["M"], lay["flat"], lay["batch"], lay["n"], lay["FB"], lay["shared_points"]) == (x.c, fmt.M, int(x.flat), x.batch, x.n, P["FB"], x.shared)
    # the sort's output is the restated one (test_gpu_msm_sort_stage checks it in depth): same counts, every run the expected set
    assert (S.read(g, lay, "count") == count).all() and S.read(g, lay, "start").tolist() == start
    order = S.read(g, lay, "sorted")
    ts = x.n if x.flat else 0
    ofb, orun, oent = S.observed_runs(order, count, x.flat, lay["CH"], lay["per"], ts)
    cfb, crun, cent = S.observed_runs(np.array(canon, dtype=np.uint32), count, x.flat, lay["CH"], lay["per"], ts)
    o, c = np.lexsort((oent, orun, ofb)), np.lexsort((cent, crun, cfb))
    assert (orun == crun).all() and (oent[o] == cent[c]).all()
    # the replay over the order the scatter produced: the same bucket logs (Case.replay asserts them against the reference) and the classes the case is for
    logs, ev = x.replay(order.tolist())
    assert not x.must - set(k for k in ev if ev[k]), ("the observed order misses", sorted(x.must - set(ev), key=str))
    # every bucket of every instance, bit for bit
    aff, raw = S.read(g, lay, "aff"), S.read(g, lay, "raw")
    want = np.zeros((P["FB"], 16), dtype=np.uint32)
    for fb, k in logs.items():
        want[fb] = multiples(k)
    bad = np.flatnonzero((aff != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} buckets differ from (log) G, first {[(int(f), int(count[f]), logs.get(int(f))) for f in bad[:8]]}"
    empty = np.flatnonzero(count == 0)
    assert not raw[empty, 20:30].any() and not aff[empty].any(), "an empty bucket is infinity"
    inf = np.array([f for f, k in logs.items() if k is None], dtype=np.int64)
    assert inf.size and not raw[inf, 20:30].any()
    assert raw[np.flatnonzero((want != 0).any(axis=1)), 20:30].any(axis=1).all()
    # the stored form every reader of the bucket array relies on (csrc/ec.hip.h; magnitude m of csrc/fq26.hip.h: limbs 0 .. 8 <= 2 m (2^26 - 1), limb 9 <=
    # 2 m (2^22 - 1)): X <= 5, Y <= 3, ZZ and ZZZ <= 1 - of every bucket, on every route
    for at, m in ((0, 5), (10, 3), (20, 1), (30, 1)):
        assert (raw[:, at:at + 9] <= 2 * m * ((1 << 26) - 1)).all() and (raw[:, at + 9] <= 2 * m * ((1 << 22) - 1)).all(), ("magnitude", at, m)
    if x.want["fq29"]:
        # what k_acc_points_sized29 stores itself (xyzz29_to_xyzz: a bucket that is one item) has every limb below 2^26; a bucket of several pieces is the sum
        # k_merge_heavy<true> makes of them with xyzz_add_chain, in the lazy bounds above
        assert (raw[count <= CAP] < (1 << 26)).all()
    # the final points: (sum s_i k_i) G
    for b in range(x.batch):
        lg = x.logs if x.shared == 1 else x.logs[(b // (x.shared or 1)) * x.n:][:x.n]
        k = sum(s * l for s, l in zip(x.rows[b], lg)) % N
        p = got_pts[b]
        assert (np.zeros(16, dtype=np.uint32) if p is None else np.frombuffer(p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little"), dtype=np.uint32)).tolist() == \
            multiples(k or None).tolist(), (name, b)


# ----------------------------------------------------------------------------- k_msm_small: its LDS sort cannot be read back; order-free constructions, by result
def _small_terms(seed):
    """buckets of window w of the 6-bit small route whose sum is the same in every order, each reaching a same-x or same-y branch in any order: {A, B, -(A + B)},
    {A, A}, {A, -A}, all equal, {A, lambda A}, {A, lambda A, lambda^2 A} (sum: infinity), points at infinity"""
    rnd = random.Random(seed)
    f6 = _fmt(6, 1, False)
    terms = []
    for w in range(41):                                             # the windows of 6 bits
        for d in range(1, 31):
            a, b = rnd.randrange(1, 50), rnd.randrange(51, 99)
            multi = rnd.choice(([a, b, -a - b], [a, a], [a, -a], [a] * 9, [a, _lam(a)], [a, _lam(a), _lam(a, 2)], [0, a, 0], [a, b, -a - b, a], [-a] * 5 + [5 * a]))
            for k in multi:
                s = f6.scalar(d, w)
                terms.append((N - s, -k) if rnd.random() < 0.3 else (s, k))
    rnd.shuffle(terms)
    return terms


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,slices", [(1, 701, 1), (2, 1499, 3), (3, 4001, 4)])
def test_small_route_by_result(gpu, oracle_lib, multiples, seed, n, slices):
    """one slice (701 terms), three of 512 (1499 terms) and four of 1024 (4001 terms): the small route's result is (sum s_i k_i) G; the reduce report names the route"""
    from test_gpu_msm_reduce_known_logs import SMALL, _report
    terms = _small_terms(seed)[:n]
    assert len(terms) == n
    sc = np.frombuffer(b"".join(s.to_bytes(32, "little") for s, _ in terms), dtype=np.uint64).reshape(-1, 4).copy()
    pts = np.stack([multiples(k % N or None) for _, k in terms]).view(np.uint64).reshape(-1, 8).copy()
    got = gpu.msm(sc, pts)
    rep = _report(gpu)
    assert rep["route"] == SMALL and rep["c"] == 6 and rep["S"] == slices
    k = sum(s * l for s, l in terms) % N
    assert got == (oracle_lib.mul(k, G1) if k else None)
