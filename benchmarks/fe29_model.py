#!/usr/bin/env python3
"""Bit-exact Python model of csrc/fq29.hip.h and of the mixed additions (complete, and exception-free with one fold for Y3) of csrc/ec29.hip.h (Fq in 9 x 29-bit limbs, lazy magnitudes), with
assertions that every intermediate fits the 32 / 64-bit register it lives in on the GPU:  python benchmarks/fe29_model.py
One branch is modelled by value only: the P = Q doubling, which the device runs on 10 x 26 limbs (xyzz_dbl_aff of ec.hip.h) and hands back
normalised; xyzz_dbl_aff here returns the same canonical limbs from plain integers.

Magnitude rule: a value has magnitude m when limb[i] <= m * B29 for i < 8 and limb[8] <= m * B24, with B29 = 2^29 + 2^8 and
B24 = 2^24 + 2^8 (the 2^8 is the slack of "tight": a weak pass leaves up to 8 in limb 8 above 2^24, a product up to 2^29 in limb 3).
tight = magnitude 1; the largest magnitude a u32 limb holds is 7.  mul takes magnitudes whose product is <= 7, sqr magnitudes <= 2; both
return tight values.  sub<K> takes a subtrahend of magnitude <= K and adds K + 1 to the magnitude of the minuend.

Every routine runs in two modes.  Exact: the device's integers, limb for limb.  Bound (bound=True): every limb is an UPPER BOUND of the
device's, a masked value is bounded by min(value, mask), a subtraction by its minuend plus the multiple of p; all other operations are
monotone, so each accumulator of the bound run bounds the same accumulator of every exact run within the input magnitudes, and the 64 / 32-bit
assertions on the bound run hold for all of them."""
import random

P = 2**256 - 2**32 - 977
M29 = (1 << 29) - 1
M24 = (1 << 24) - 1
B29 = (1 << 29) + (1 << 8)
B24 = (1 << 24) + (1 << 8)
R0, R1 = 0x7A20, 0x100          # 2^261 = R1 * 2^29 + R0 (mod p)
PL = [0x1FFFFC2F, 0x1FFFFFF7] + [M29] * 6 + [M24]   # limbs of p
U64 = (1 << 64) - 1
MAX_MAG = 7

assert sum(v << (29 * i) for i, v in enumerate(PL)) == P and (R1 << 29) + R0 == (1 << 261) % P


class Overflow(AssertionError):
    pass


def u64(x):
    if not 0 <= x <= U64:
        raise Overflow(f"64-bit overflow: {x.bit_length()} bits")
    return x


def u32(x):
    if not 0 <= x < (1 << 32):
        raise Overflow(f"32-bit overflow: {x.bit_length()} bits")
    return x


def val(a):
    return sum(v << (29 * i) for i, v in enumerate(a))


def from_int(x):
    assert 0 <= x < (1 << 261)
    return [(x >> (29 * i)) & M29 for i in range(9)]


def mag_limbs(m):
    """the largest limbs of magnitude m"""
    return [m * B29] * 8 + [m * B24]


def mag_ok(a, m):
    return all(x <= y for x, y in zip(a, mag_limbs(m)))


def mag_of(a):
    return next(m for m in range(0, 64) if mag_ok(a, m))


def _lo(x, mask, bound):
    return min(x, mask) if bound else x & mask


def _mul_tail(r, c, t8, u8, u7, bound):
    """limb 8 and everything above 2^256 folded back (2^256 = 2^32 + 0x3D1 = 8 * 2^29 + 977)"""
    c = u64(c + t8 + u64(u8 * R0) + u64(u7 * R1))
    r[8] = _lo(c, M24, bound)
    top = u64((c >> 24) + u64(u64(u8 * R1) << 5))      # units of 2^256
    c = u64(r[0] + u64(top * 0x3D1)); r[0] = _lo(c, M29, bound); c >>= 29
    c = u64(c + r[1] + u64(top << 3)); r[1] = _lo(c, M29, bound); c >>= 29
    c = u64(c + r[2]); r[2] = _lo(c, M29, bound); c >>= 29
    r[3] = u32(r[3] + c)
    if not mag_ok(r, 1):
        raise Overflow(f"product not tight: {r}")
    return r


def _product(col, bound):
    """the two carry chains of fq29_mul / fq29_sqr over the column sums col(k, acc)"""
    d = col(8, 0)
    t8 = _lo(d, M29, bound); d >>= 29
    u = []
    for k in range(9, 17):
        d = col(k, d)
        u.append(_lo(d, M29, bound)); d >>= 29
    u8 = d                           # leftover carry
    if u8 >= (1 << 36):
        raise Overflow("leftover carry of the high chain")
    r = [0] * 9
    c = 0
    for k in range(8):
        c = col(k, c)
        c = u64(c + u[k] * R0)
        if k:
            c = u64(c + u[k - 1] * R1)
        r[k] = _lo(c, M29, bound); c >>= 29
    return _mul_tail(r, c, t8, u8, u[7], bound)


def mul(a, b, bound=False):
    """magnitudes with product <= 7 in, tight out (the assertions decide, not this sentence)"""
    for x in list(a) + list(b):
        u32(x)

    def col(k, acc):
        for i in range(max(0, k - 8), min(8, k) + 1):
            acc = u64(acc + a[i] * b[k - i])
        return acc
    return _product(col, bound)


def sqr(a, bound=False):
    """magnitude <= 2 in, tight out: 45 products, the off-diagonal ones on the doubled limb"""
    a2 = [u32(x << 1) for x in a]

    def col(k, acc):
        i = max(0, k - 8)
        while 2 * i < k:
            acc = u64(acc + a2[i] * a[k - i]); i += 1
        if k % 2 == 0:
            acc = u64(acc + a[k // 2] * a[k // 2])
        return acc
    return _product(col, bound)


def mul_add2(a, b, c, d, bound=False):
    """a b + c d in one pair of chains: both products' terms go into each column, one fold and one tail.  mag(a) mag(b) + mag(c) mag(d) <= 7
    in, tight out: column 7 then holds 16 products of at most 7 * 8 * B29^2 together, what mul's 8 hold at 1 * 7 (the assertions decide)"""
    for x in list(a) + list(b) + list(c) + list(d):
        u32(x)

    def col(k, acc):
        for i in range(max(0, k - 8), min(8, k) + 1):
            acc = u64(acc + a[i] * b[k - i])
        for i in range(max(0, k - 8), min(8, k) + 1):
            acc = u64(acc + c[i] * d[k - i])
        return acc
    return _product(col, bound)


def add(a, b, bound=False):
    return [u32(x + y) for x, y in zip(a, b)]


def sub(a, b, K, bound=False):
    """a - b for b of magnitude <= K; magnitude mag(a) + K + 1"""
    if not mag_ok(b, K):
        raise Overflow(f"subtrahend above magnitude {K}")
    kp = [(K + 1) * PL[i] for i in range(9)]
    assert all(kp[i] >= mag_limbs(K)[i] for i in range(9))      # no limb goes negative
    if bound:
        return [u32(a[i] + kp[i]) for i in range(9)]
    return [u32(a[i] + u32(kp[i] - b[i])) for i in range(9)]


def neg(a, K, bound=False):
    return sub([0] * 9, a, K, bound)


def mul_int(a, k, bound=False):
    return [u32(x * k) for x in a]


def weak_pass(a, bound=False):
    """one folding pass, any magnitude <= 7: limbs 0 .. 7 < 2^29, limb 8 <= 2^24 + 7 (tight); the value is < 2^256 + 2^236"""
    t = [u32(x) for x in a]
    x = t[8] >> 24; t[8] = _lo(t[8], M24, bound)
    t[0] = u32(t[0] + x * 0x3D1); t[1] = u32(t[1] + (x << 3))
    for i in range(8):
        t[i + 1] = u32(t[i + 1] + (t[i] >> 29)); t[i] = _lo(t[i], M29, bound)
    if not mag_ok(t, 1):
        raise Overflow("weak pass not tight")
    return t


def weak_is_zero(t):
    """on a weak-passed value: 0 (mod p) is all limbs zero or exactly the limbs of p (the value is below 2 p and limbs 0 .. 7 are below 2^29)"""
    z0, z1 = 0, M29
    for i in range(9):
        z0 |= t[i]
        z1 &= t[i] ^ (PL[i] ^ M29)
    return z0 == 0 or z1 == M29


def normalizes_to_zero(a):
    return weak_is_zero(weak_pass(a))


def to_fq26(a, bound=False):
    """weak pass, then the same bits cut into 10 x 26: every limb below 2^26, magnitude 1 of fq26.hip.h"""
    t = weak_pass(a, bound)
    if bound:
        return [(1 << 26) - 1] * 9 + [t[8] >> 2]
    out = []
    for j in range(10):
        s, off = divmod(26 * j, 29)
        v = t[s] >> off
        if off + 26 > 29 and s + 1 < 9:
            v |= u32((t[s + 1] << (29 - off)) & 0xFFFFFFFF)
        out.append(v & ((1 << 26) - 1) if j < 9 else v)
    assert all(x < (1 << 26) for x in out) and out[9] <= 2 * ((1 << 22) - 1)
    assert sum(x << (26 * j) for j, x in enumerate(out)) == val(t)
    return out


def from_fe(words):
    """canonical 8 x 32 words -> 9 x 29"""
    v = sum(w << (32 * i) for i, w in enumerate(words))
    assert v < (1 << 256)
    return from_int(v)


def canonical(a):
    return val(a) % P


# ---- the group law of ec29.hip.h: affine (x, y) of magnitudes 1 and <= 2, accumulator (X <= 5, Y <= 3, ZZ = ZZZ = 1); infinity: ZZ all zero
def is_zero_limbs(a):
    return not any(a)


def xyzz_inf():
    return [[0] * 9 for _ in range(4)]


def xyzz_from_aff(q):
    inf = is_zero_limbs(q[0]) and is_zero_limbs(q[1])
    one = [0 if inf else 1] + [0] * 8
    return [list(q[0]), list(q[1]), list(one), list(one)]


def xyzz_dbl_aff(q, bound=False):
    """the P = Q branch: the device repacks the point into 10 x 26 limbs, doubles it there (xyzz_dbl_aff of ec.hip.h, mdbl-2008-s-1) and cuts the
    normalised result back into 29-bit limbs, so the output is the canonical value of each coordinate"""
    if bound:
        to_fq26(q[0], True); to_fq26(q[1], True)
        return [[M29] * 8 + [M24] for _ in range(4)]               # canonical: every limb below its width
    x, y = val(q[0]) % P, val(q[1]) % P
    if (is_zero_limbs(q[0]) and is_zero_limbs(q[1])) or y == 0:
        return xyzz_inf()
    U = 2 * y % P
    V = U * U % P; W = U * V % P; S = x * V % P; Mm = 3 * x * x % P
    X = (Mm * Mm - 2 * S) % P
    Y = (Mm * (S - X) - W * y) % P
    return [from_int(X), from_int(Y), from_int(V), from_int(W)]


def xyzz_madd(acc, q, bound=False):
    """acc += q, complete (madd-2008-s); the magnitudes in the comments are asserted below"""
    X, Y, ZZ, ZZZ = acc
    if not bound:
        if is_zero_limbs(q[0]) and is_zero_limbs(q[1]):
            return acc
        if is_zero_limbs(ZZ):
            return xyzz_from_aff(q)
    assert mag_ok(X, 5) and mag_ok(Y, 3) and mag_ok(ZZ, 1) and mag_ok(ZZZ, 1) and mag_ok(q[0], 1) and mag_ok(q[1], 2)
    U2 = mul(q[0], ZZ, bound); S2 = mul(q[1], ZZZ, bound)
    Pd = sub(U2, X, 5, bound)                                  # 1 + 6 = 7
    R = sub(S2, Y, 3, bound)                                   # 1 + 4 = 5
    assert mag_ok(Pd, 7) and mag_ok(R, 5)
    Pw = weak_pass(Pd, bound); Rw = weak_pass(R, bound)        # both tight: sqr takes <= 2
    if not bound and weak_is_zero(Pw):
        return xyzz_dbl_aff(q) if weak_is_zero(Rw) else xyzz_inf()
    PP = sqr(Pw, bound); PPP = mul(Pw, PP, bound); Q = mul(X, PP, bound)        # 5 * 1
    X3 = sub(sqr(Rw, bound), add(PPP, mul_int(Q, 2, bound), bound), 3, bound)   # 1 + 4 = 5
    T = sub(Q, X3, 5, bound)                                   # 1 + 6 = 7
    assert mag_ok(T, 7)
    Y3 = sub(mul(Rw, T, bound), mul(Y, PPP, bound), 1, bound)  # 1 * 7, 3 * 1; 1 + 2 = 3
    out = [X3, Y3, mul(ZZ, PP, bound), mul(ZZZ, PPP, bound)]
    assert mag_ok(out[0], 5) and mag_ok(out[1], 3) and mag_ok(out[2], 1) and mag_ok(out[3], 1)
    return out


def _y3(Rw, Q, X3, Y, PPP, KY, bound):
    """Y3 = R (Q - X3) - Y PPP as ONE reduced sum of two products (mul_add2): Q - X3 (1 + 6 = 7) takes a weak pass so that the pair stays
    inside 1 * 1 + (KY + 1) * 1 <= 7; tight out"""
    T = sub(Q, X3, 5, bound)
    assert mag_ok(T, 7)
    return mul_add2(Rw, weak_pass(T, bound), neg(Y, KY, bound), PPP, bound)


def xyzz_madd_fast(acc, q, bound=False):
    """acc += q for acc and q finite and q != +-acc: madd-2008-s with no test at all.  On any other input the limbs stay inside the same
    bounds (they depend on the magnitudes alone) and ZZ3 = ZZ Pd^2 = 0 (mod p) from then on: the caller tests ZZ once per item"""
    X, Y, ZZ, ZZZ = acc
    assert mag_ok(X, 5) and mag_ok(Y, 3) and mag_ok(ZZ, 1) and mag_ok(ZZZ, 1) and mag_ok(q[0], 1) and mag_ok(q[1], 2)
    U2 = mul(q[0], ZZ, bound); S2 = mul(q[1], ZZZ, bound)
    Pw = weak_pass(sub(U2, X, 5, bound), bound); Rw = weak_pass(sub(S2, Y, 3, bound), bound)        # 7 -> 1, 5 -> 1
    PP = sqr(Pw, bound); PPP = mul(Pw, PP, bound); Q = mul(X, PP, bound)                            # 5 * 1
    X3 = sub(sqr(Rw, bound), add(PPP, mul_int(Q, 2, bound), bound), 3, bound)                       # 1 + 4 = 5
    Y3 = _y3(Rw, Q, X3, Y, PPP, 3, bound)                                                           # 1 * 1 + 4 * 1 = 5 -> 1
    out = [X3, Y3, mul(ZZ, PP, bound), mul(ZZZ, PPP, bound)]
    assert mag_ok(out[0], 5) and mag_ok(out[1], 1) and mag_ok(out[2], 1) and mag_ok(out[3], 1)
    return out


def xyzz_from_two(p, q, bound=False):
    """p + q for two finite affine points of different x (mmadd-2008-s, 4 M + 2 S), y magnitudes <= 2; x1 = x2 gives ZZ = 0 (mod p)"""
    assert mag_ok(p[0], 1) and mag_ok(p[1], 2) and mag_ok(q[0], 1) and mag_ok(q[1], 2)
    Pw = weak_pass(sub(q[0], p[0], 1, bound), bound); Rw = weak_pass(sub(q[1], p[1], 2, bound), bound)    # 3 -> 1, 5 -> 1
    PP = sqr(Pw, bound); PPP = mul(Pw, PP, bound); Q = mul(p[0], PP, bound)
    X3 = sub(sqr(Rw, bound), add(PPP, mul_int(Q, 2, bound), bound), 3, bound)                       # 1 + 4 = 5
    Y3 = _y3(Rw, Q, X3, p[1], PPP, 2, bound)                                                        # 1 * 1 + 3 * 1 = 4 -> 1
    out = [X3, Y3, PP, PPP]
    assert mag_ok(out[0], 5) and mag_ok(out[1], 1) and mag_ok(out[2], 1) and mag_ok(out[3], 1)
    return out


def item_fast(points, bound=False, two=True):
    """one item of k_acc_points_sized29_fast: entries (0, 0) skipped, the sum started from the first two finite ones through from_two (two=False:
    from the first alone), the rest through madd_fast, one zero test of ZZ at the end; a flagged item is redone with the complete addition"""
    fin = [q for q in points if not (is_zero_limbs(q[0]) and is_zero_limbs(q[1]))]
    if not fin:
        return xyzz_inf()
    if two and len(fin) > 1:
        acc, rest = xyzz_from_two(fin[0], fin[1], bound), fin[2:]
    else:
        acc, rest = xyzz_from_aff(fin[0]), fin[1:]
    for q in rest:
        acc = xyzz_madd_fast(acc, q, bound)
    if normalizes_to_zero(acc[2]):
        acc = xyzz_inf()
        for q in points:
            acc = xyzz_madd(acc, q)
    return acc


def xyzz_affine(acc):
    """canonical affine integers of an accumulator, None for infinity"""
    X, Y, ZZ, ZZZ = (val(c) % P for c in acc)
    if is_zero_limbs(acc[2]):
        return None
    return X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P


# ---- plain integers, for comparison
def ec_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % P == 0:
            return None
        lam = 3 * p[0] * p[0] * pow(2 * p[1], -1, P) % P
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, P) % P
    x = (lam * lam - p[0] - q[0]) % P
    return x, (lam * (p[0] - x) - p[1]) % P


def rand_point(rnd):
    while True:
        x = rnd.randrange(P)
        y2 = (x * x * x + 7) % P
        y = pow(y2, (P + 1) // 4, P)
        if y * y % P == y2:
            return x, y


def rand_mag(rnd, m):
    return [rnd.randrange(v + 1) for v in mag_limbs(m)]


def check_bounds():
    """the worst case of every routine at its contract"""
    for ma, mb in [(1, 7), (7, 1), (1, 1), (2, 3), (3, 2), (5, 1), (1, 5)]:
        mul(mag_limbs(ma), mag_limbs(mb), bound=True)
        mul(mag_limbs(ma), mag_limbs(mb))                       # the same limbs through the exact chains
    for m in (1, 2):
        sqr(mag_limbs(m), bound=True); sqr(mag_limbs(m))
    for m in range(1, MAX_MAG + 1):
        weak_pass(mag_limbs(m), bound=True); to_fq26(mag_limbs(m), bound=True); to_fq26(mag_limbs(m))
    for K in range(1, MAX_MAG):
        for ma in range(0, MAX_MAG - K):
            assert mag_ok(sub(mag_limbs(ma), [0] * 9, K), ma + K + 1)
    acc = [mag_limbs(5), mag_limbs(3), mag_limbs(1), mag_limbs(1)]
    q = [mag_limbs(1), mag_limbs(2)]
    xyzz_madd(acc, q, bound=True)
    d = xyzz_dbl_aff(q, bound=True)
    assert mag_ok(d[0], 5) and mag_ok(d[1], 3) and mag_ok(d[2], 1) and mag_ok(d[3], 1)
    for ma, mb, mc, md in MUL_ADD2_WORST:
        assert ma * mb + mc * md == 7
        mul_add2(mag_limbs(ma), mag_limbs(mb), mag_limbs(mc), mag_limbs(md), bound=True)
        mul_add2(mag_limbs(ma), mag_limbs(mb), mag_limbs(mc), mag_limbs(md))
    xyzz_madd_fast(acc, q, bound=True)
    xyzz_from_two(q, q, bound=True)


MUL_ADD2_WORST = [(1, 1, 1, 6), (1, 3, 4, 1), (1, 1, 3, 2), (2, 2, 1, 3), (1, 6, 1, 1), (7, 1, 0, 0), (1, 4, 3, 1), (5, 1, 1, 2)]


def forbidden_pairs_trip():
    """mul(1, 8) and mul(2, 4) reach 2^64 in column 7: the overflow assertion must fire"""
    try:
        mul_add2(mag_limbs(1), mag_limbs(4), mag_limbs(4), mag_limbs(1))
    except Overflow:
        pass
    else:
        raise AssertionError("mul_add2 at 1 * 4 + 4 * 1 did not trip the overflow assertion")
    for ma, mb in [(1, 8), (2, 4)]:
        a, b = mag_limbs(ma), mag_limbs(mb)
        if mb == 8:
            b = [min(v, (1 << 32) - 1) for v in b]             # a u32 holds no more
        try:
            mul(a, b)
        except Overflow:
            continue
        raise AssertionError(f"mul({ma}, {mb}) did not trip the overflow assertion")
    try:
        sqr(mag_limbs(3))
    except Overflow:
        return
    raise AssertionError("sqr(3) did not trip the overflow assertion")


def main():
    rnd = random.Random(29)
    check_bounds()
    forbidden_pairs_trip()
    for it in range(10000):
        ma = rnd.choice([1, 2, 3, 5, 7])
        mb = rnd.choice([m for m in [1, 2, 3, 5, 7] if m * ma <= 7])
        a, b = rand_mag(rnd, ma), rand_mag(rnd, mb)
        if it % 7 == 0:
            a = from_int(rnd.choice([0, 1, P - 1, P, P - 2, 2**256 - 1]))
        r = mul(a, b)
        assert val(r) % P == val(a) * val(b) % P
        if mag_ok(a, 2):
            assert val(sqr(a)) % P == val(a) ** 2 % P
        w = weak_pass(a)
        assert val(w) % P == val(a) % P and val(w) < 2**256 + 2**236
        assert weak_is_zero(w) == (val(a) % P == 0)
        assert sum(x << (26 * j) for j, x in enumerate(to_fq26(a))) % P == val(a) % P
        if ma + mb + 1 <= MAX_MAG:
            assert val(sub(a, b, mb)) % P == (val(a) - val(b)) % P
            assert val(add(a, b)) % P == (val(a) + val(b)) % P
    for a in ([0] * 9, PL, [2 * x for x in PL], [3 * x for x in PL]):
        assert normalizes_to_zero(a)
    assert not normalizes_to_zero(from_int(1)) and not normalizes_to_zero(from_int(P - 1)) and not normalizes_to_zero(from_int(P + 1))
    # chains of mixed additions against integers: random, P + P, P - P, infinity in the chain
    for it in range(40):
        pts = [rand_point(rnd) for _ in range(6)]
        chain = [pts[0], pts[1], pts[1], pts[2], None, (pts[2][0], P - pts[2][1]), pts[3], pts[4], pts[5]]
        if it % 4 == 1:
            chain = [pts[0], pts[0], (pts[0][0], P - pts[0][1]), (pts[0][0], P - pts[0][1]), pts[1]]    # P, P, -P, -P, Q
        acc, ref = xyzz_inf(), None
        for pt in chain:
            q = [from_int(0), from_int(0)] if pt is None else [from_int(pt[0]), from_int(pt[1])]
            if pt is not None and rnd.random() < 0.5:                # the sign fold: y as 2 p - (p - y)
                q[1] = neg(from_int(P - pt[1]), 1)
            acc = xyzz_madd(acc, q)
            ref = ec_add(ref, pt)
            assert xyzz_affine(acc) == ref
    # mul_add2 by value, inside and at its contract
    for it in range(3000):
        ma, mb, mc, md = rnd.choice(MUL_ADD2_WORST + [(1, 1, 4, 1), (1, 1, 3, 1), (1, 1, 1, 1)])
        a, b, c, d = rand_mag(rnd, ma), rand_mag(rnd, mb), rand_mag(rnd, mc), rand_mag(rnd, md)
        if it % 5 == 0:
            a, b, c, d = mag_limbs(ma), mag_limbs(mb), mag_limbs(mc), mag_limbs(md)
        assert val(mul_add2(a, b, c, d)) % P == (val(a) * val(b) + val(c) * val(d)) % P
    # the fast item against integers: ordinary items limb for limb the group element of the complete chain, exceptions at every position redone
    for it in range(60):
        pts = [rand_point(rnd) for _ in range(6)]
        m = lambda pt: (pt[0], P - pt[1])
        chain = [[pts[0]], pts[:2], pts[:3], pts, [pts[0], pts[0]], [pts[0], m(pts[0])], [pts[0], pts[1], pts[1]], [pts[0], pts[1], m(pts[1]), pts[2]],
                 [pts[0], m(pts[0]), pts[1], pts[2]], pts[:5] + [pts[4]], pts[:5] + [m(pts[4])], [None, pts[0], None, pts[1], pts[2], None], [None, None],
                 [pts[0], None, m(pts[0])], [pts[0], pts[0], pts[1], m(pts[1]), pts[2]]][it % 15]
        item, ref = [], None
        for pt in chain:
            q = [from_int(0), from_int(0)] if pt is None else [from_int(pt[0]), from_int(pt[1])]
            if pt is not None and rnd.random() < 0.5:
                q[1] = neg(from_int(P - pt[1]), 1)
            item.append(q)
            ref = ec_add(ref, pt)
        assert xyzz_affine(item_fast(item)) == ref and xyzz_affine(item_fast(item, two=False)) == ref
    # a lane gone wrong (ZZ = 0 mod p after P = +-Q) keeps ZZ = 0 and every bound to the end of its item
    p0, rest = rand_point(rnd), [rand_point(rnd) for _ in range(8)]
    for second in (p0, (p0[0], P - p0[1])):
        acc = xyzz_madd_fast(xyzz_from_aff([from_int(p0[0]), from_int(p0[1])]), [from_int(second[0]), from_int(second[1])])
        for pt in rest:
            assert normalizes_to_zero(acc[2])
            acc = xyzz_madd_fast(acc, [from_int(pt[0]), from_int(pt[1])])
        assert normalizes_to_zero(acc[2])
    print("fe29 model OK")


if __name__ == "__main__":
    main()
