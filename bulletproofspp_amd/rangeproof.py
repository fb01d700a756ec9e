"""Typed reciprocal range proofs (RangeProof.TypedReciprocal + RangeProof.Internal + the generic RangeProof wrapper of the
reference) on top of the GPU norm-linear argument — SURVEY.md section 8(f) rank 1.

This is HOST protocol logic (phase 1-3 commitments' scalars, blinding algebra, public constants); everything that touches
curve points goes through a `Backend`: `commit` (the reference's `commitRPW` = one Pedersen MSM, src/RangeProof/Internal.hs:45-50)
and the norm-linear argument's prover / verifier (src/Bulletproof.hs:346-378).  `GpuBackend` is the product backend (C ABI:
bppp_msm, bppp_nl_*); there is no CPU backend in the package — the tests inject one built from `oracle/` to check that the GPU
path yields the same transcript bit for bit.

Names follow the reference so the call sites read like src/RangeProof/TypedReciprocal.hs.  Both argument flavours are wired:
"NL" (Bulletproof.NormArgument; `examples/{32by64,64by64,96by64,128by64}`) and "IP" (Bulletproof.InnerProductArgument, the
schema default, app/Parse.hs:100; `examples/{32bit,64bit,rec_test}`).  The reference cannot be run here (no GHC), so proofs are
pinned by algebraic closure (prove -> verify accepts; any tampering rejects) and by the shapes of SURVEY.md Appendix B, not by
reference-generated vectors: parity of this layer with the Haskell implementation is UNPINNED.
"""
from __future__ import annotations

import contextlib
import hashlib
import os
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141      # group order: the scalar field `s`
Point = Optional[Tuple[int, int]]
OracleN = Callable[[List[Point], int], List[int]]     # whole transcript (newest first), count -> that many challenges
RandFn = Callable[[int], int]                         # counter -> scalar (ZKPT's `h n`, src/ZKP.hs:88-92)


def decode_field(b: bytes, modulus: int) -> int:
    """`decode` through Binary (Prime p) (src/Encoding.hs:75-79): four big-endian 64-bit words, LEAST-significant word first,
    reduced by toP.  This is how the reference turns a SHA-256 digest into a field element (`hash = decode . SHA.hash`,
    app/Main.hs:64-65) and how it reads scalars and coordinates from files."""
    return sum(int.from_bytes(b[8 * i:8 * i + 8], "big") << (64 * i) for i in range(4)) % modulus


# ----------------------------------------------------------------------------- small helpers (src/Utils.hs)
def inv(a: int) -> int:
    a %= N
    return pow(a, N - 2, N) if a else 0


def batch_inverse(xs: Sequence[int]) -> List[int]:
    """batchInverse (src/Data/Field/BatchInverse.hs:18-39): Montgomery's trick, 0 -> 0."""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        if x % N:
            acc = acc * x % N
    y = inv(acc)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        if xs[i] % N:
            out[i] = y * pre[i] % N
            y = y * xs[i] % N
    return out


def powers1(a: int, n: int) -> List[int]:
    """first n of powers' a = [a, a^2, ...] (Utils.hs:107-108)"""
    out, c = [], 1
    for _ in range(n):
        c = c * a % N
        out.append(c)
    return out


def integer_log(b: int, n: int) -> int:
    """integerLog (Utils.hs:78-79)"""
    r = 0
    while n >= b:
        n //= b
        r += 1
    return r


def pad_right(n: int, z, xs: Sequence) -> list:
    return (list(xs) + [z] * n)[:n]


def insert_at(n: int, x, xs: Sequence) -> list:
    xs = list(xs)
    return xs[:n] + [x] + xs[n:]


def remove_at(n: int, xs: Sequence) -> list:
    xs = list(xs)
    return xs[:n] + xs[n + 1:]


# ----------------------------------------------------------------------------- RPWitness (RangeProof/Internal.hs:20-43)
@dataclass
class RPW:
    sc: int = 0
    lin: List[int] = field(default_factory=list)
    nrm: List[int] = field(default_factory=list)

    def __add__(self, o: "RPW") -> "RPW":        # (^+^) = zipWithDef'' (+) 0 0
        z = lambda a, b: [((a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0)) % N for i in range(max(len(a), len(b)))]
        return RPW((self.sc + o.sc) % N, z(self.lin, o.lin), z(self.nrm, o.nrm))

    def scale(self, s: int) -> "RPW":            # (*^)
        return RPW(self.sc * s % N, [x * s % N for x in self.lin], [x * s % N for x in self.nrm])


# ----------------------------------------------------------------------------- ranges and digits (TypedReciprocal.hs:77-131)
@dataclass
class RangeData:
    base: int
    lo: int
    hi: int
    is_shared: bool
    is_output: bool
    is_assumed: bool
    has_bit: bool
    base_coeffs: List[int]


def make_range_data(base: int, lo: int, hi: int, is_shared: bool = False, is_output: bool = False, is_assumed: bool = False) -> Optional[RangeData]:
    """makeRangeData (TypedReciprocal.hs:103-120) for the field of characteristic N; None if the range is invalid."""
    if not (hi > lo and base > 1 and hi - lo < N):
        return None
    b, w = base, hi - lo
    n1 = integer_log(b, w - 1)
    has_bit = ((w - 1) % (b - 1)) != 0
    tail = [b ** (n1 - i) for i in range(1, n1 + 1)]
    if not has_bit:
        bs = [(w - b ** n1) // (b - 1)] + tail
    elif w < 2 * b ** n1:
        bs = [w - b ** n1] + tail
    else:
        bn1 = 1 + w // (2 * (b - 1)) - (b ** n1 - 1) // (b - 1)
        bs = [w - bn1 * (b - 1) - b ** n1, bn1] + tail
    return RangeData(b, lo, hi, is_shared, is_output, is_assumed, has_bit, [] if is_assumed else bs)


def digits(rd: RangeData, n: int) -> List[int]:
    """digits (TypedReciprocal.hs:125-127): greedy mixed-radix digits; the first is binary when has_bit."""
    out = []
    for i, coeff in enumerate(rd.base_coeffs):
        radix = 2 if (rd.has_bit and i == 0) else rd.base
        d = min(radix - 1, n // coeff)
        n -= d * coeff
        out.append(d)
    return out


def counts(xs: Sequence[int], ys: Sequence[int]) -> List[int]:
    m: Dict[int, int] = {}
    for y in ys:
        m[y] = m.get(y, 0) + 1
    return [m.get(x, 0) for x in xs]


# Phase1 (TypedReciprocal.hs:56-60): ("inline", idx, base, b, d, m, s) | ("shared", idx, base, b, d) | ("typing", idx, io, ia, v, t);
# private fields (d, m, v, t) are None on the verifier's side
def make_phase1s(ind: int, rd: RangeData, n: Optional[int]):
    """makePhase1s / makePhase1sVer (TypedReciprocal.hs:133-169): (phase-1 records, shared multiplicities or None)."""
    if rd.is_assumed:
        return [], None
    ver = n is None
    n_adj = 0 if ver else n - rd.lo
    if not (0 <= n_adj < rd.hi - rd.lo):
        raise ValueError("value outside its range")
    b = rd.base
    ds = digits(rd, n_adj)
    ms = ([ds[0]] + counts(range(1, b), ds[1:])) if rd.has_bit else counts(range(1, b), ds)
    ns = ([1] if rd.has_bit else []) + list(range(1, b))
    radix = lambda i: 2 if (rd.has_bit and i == 0) else b
    priv = (lambda v: None) if ver else (lambda v: v % N)
    if rd.is_shared:
        ph1s = [("shared", ind, radix(i), rd.base_coeffs[i] % N, priv(ds[i])) for i in range(min(len(rd.base_coeffs), len(ds)))]
        return ph1s, (None if ver else [m % N for m in ms])
    ln = max(len(rd.base_coeffs), len(ds), len(ms), len(ns))
    bs_, ds_, ms_, ns_ = (pad_right(ln, 0, w) for w in (rd.base_coeffs, ds, ms, ns))
    return [("inline", ind, radix(i), bs_[i] % N, priv(ds_[i]), priv(ms_[i]), ns_[i] % N) for i in range(ln)], None


def get_ds_ms(ph1s) -> Tuple[List[int], List[int]]:
    """getDsMs (TypedReciprocal.hs:74-80)"""
    ds, ms = [], []
    for p in ph1s:
        if p[0] == "inline":
            ds.append(p[4]); ms.append(p[5])
        elif p[0] == "shared":
            ds.append(p[4]); ms.append(0)
        else:
            ds.append(p[5]); ms.append(0)
    return ds, ms


# Phase2 (TypedReciprocal.hs:180-181)
@dataclass
class Ph2:
    is_t: bool
    d: Optional[int]
    m: Optional[int]
    u: int
    v: int
    r: Optional[int]
    c: int


def make_phase2s(e: int, e_inv: int, x: int, base_map: Dict[int, int], ph1s, private: bool) -> List[Ph2]:
    """makePhase2s (TypedReciprocal.hs:185-205).  private=False is the verifier's `b ~ ()` instantiation."""
    dens, ss, ps, vs, rec = [], [], [], [], []
    xpow: Dict[int, int] = {}
    for p in ph1s:
        xi = xpow.get(p[1])
        if xi is None:
            xi = xpow[p[1]] = pow(x, 2 * (p[1] + 1), N)
        if p[0] == "typing":
            _, _, io, ia, v, t = p
            x2 = (-x) % N if io else x % N
            dens.append((e + t) % N if private else 0); ss.append(0); ps.append(v if private else 0); vs.append(x2)
            rec.append((True, t, 0 if private else None, 0 if ia else xi, x2))
        elif p[0] == "inline":
            _, _, base, b, d, m, s = p
            x2 = base_map[base]
            dens.append((e + d) % N if private else 0); ss.append(0 if s == 0 else (e + s) % N); ps.append(1); vs.append(x2)
            rec.append((False, d, m, xi * b % N, x2))
        else:
            _, _, base, b, d = p
            x2 = base_map[base]
            dens.append((e + d) % N if private else 0); ss.append(0); ps.append(1); vs.append(x2)
            rec.append((False, d, 0 if private else None, xi * b % N, x2))
    rs = [a * b % N for a, b in zip(ps, batch_inverse(dens))] if private else [None] * len(ph1s)
    cs = [v * (0 if s == 0 else (e_inv - s) % N) % N for v, s in zip(vs, batch_inverse(ss))]
    return [Ph2(is_t, d, m, u, v, r, c) for (is_t, d, m, u, v), r, c in zip(rec, rs, cs)]


def make_shared_coeffs(e: int, e_inv: int, m_bases: Sequence[int], base_map: Dict[int, int]) -> List[int]:
    """makeSharedCoeffs (TypedReciprocal.hs:213-216)"""
    xs, ss = [], []
    for b in m_bases:
        for s in range(1, b):
            xs.append(base_map[b]); ss.append((e + s) % N)
    return [x * ((e_inv - si) % N) % N for x, si in zip(xs, batch_inverse(ss))]


def make_error_terms(e: int, xp: int, shared_cs: Sequence[int], bls_ms: Sequence[int], ph3s) -> List[int]:
    """makeErrorTerms (TypedReciprocal.hs:226-243); ph3s = [(Ph2, q2, bl)]"""
    tot = [0, 0, 0, 2 * sum(a * b for a, b in zip(shared_cs, bls_ms)) % N, 0, 0]
    for p, q2, bl in ph3s:
        d, m, u, v, r, c = p.d, p.m, p.u, p.v, p.r, p.c
        rC = xp * (u + q2) % N if p.is_t else u
        dC = (v + q2 * e) % N
        errs = [q2 * bl * bl,
                2 * q2 * m * bl,
                q2 * m * m + 2 * bl * (q2 * d + dC),
                2 * (bl * (q2 * r + rC) + m * (q2 * d + dC)),
                (q2 * d * d + 2 * d * dC) + 2 * (bl * c + m * (q2 * r + rC)),
                (q2 * r * r + 2 * r * rC) + 2 * c * d]
        tot = [(a + b) % N for a, b in zip(tot, errs)]
    return tot


def input_coeffs(has_types: bool, assumed: Sequence[bool], x: int, q0: int) -> List[int]:
    """inputCoeffs (TypedReciprocal.hs:325-328)"""
    xp = [0 if a else p for a, p in zip(assumed, powers1(x * x % N, len(assumed)))]
    return [(a + b) % N for a, b in zip(powers1(q0, len(assumed)), xp)] if has_types else xp


def make_bp_coeffs(has_types: bool, xp: int, r0: int, r1: int, t: int, cs: Sequence[int]) -> List[int]:
    """makeBpCoeffs (TypedReciprocal.hs:391-396)"""
    rs = r0 * r1 % N
    tp = lambda k: pow(t, k, N)
    return [(-xp) % N if has_types else 0, rs * t % N, rs * tp(2) % N, rs * tp(3) % N, r0 * tp(4) % N, rs * tp(6) % N] + \
           [2 * tp(3) * c % N for c in cs]


def make_public_consts(e: int, e_inv: int, x: int, xp: int, q0: int, q0_inv: int, t: int, has_types: bool, rds: Sequence[RangeData],
                       pub_vt: Sequence[Tuple[bool, int, int]], ph2s: Sequence[Ph2]) -> RPW:
    """makePublicConsts (TypedReciprocal.hs:246-274); pub_vt entries are (isOutput, type, amount) as destructured at :258."""
    t2, t3, t4, t5 = (pow(t, k, N) for k in (2, 3, 4, 5))
    mins = [0 if rd.is_assumed else rd.lo % N for rd in rds]
    pub_rs = batch_inverse([(e + ty) % N for _, ty, _ in pub_vt])
    pub_sum = sum(((-r * v) if is_out else (r * v)) for (is_out, _, v), r in zip(pub_vt, pub_rs)) % N
    z = -2 * t5 * sum(a * b for a, b in zip(mins, powers1(x * x % N, len(mins))))
    if has_types:
        z -= 2 * t5 * x * pub_sum
    ts0, ts1 = [], []
    for p, q2, qi2 in zip(ph2s, powers1(q0, len(ph2s)), powers1(q0_inv, len(ph2s))):
        if p.is_t:
            rC, p2C = xp * (qi2 * p.u + 1) % N, 0
        else:
            rC, p2C = qi2 * p.u % N, (2 * q2 + 2 * e_inv * p.v) % N
        pv = (t2 * (e + qi2 * p.v) + t3 * rC + t4 * (qi2 * p.c)) % N
        ts0.append((q2 * pv * pv + t5 * p2C) % N)
        ts1.append(pv)
    return RPW((z + sum(ts0)) % N, [], ts1)


# ----------------------------------------------------------------------------- blinding (RangeProof/Internal.hs:118-196)
def blind_witness(n: int, k: int, ls: Sequence[int], ns: Sequence[int], rnd: Callable[[], int]) -> RPW:
    """blindWitness (:130-139)"""
    n_bls = 2 * n - 1 if k == 1 else 2 * n - k + 1
    bls = pad_right(2 * n + 1, 0, insert_at(2 * n - k, 0, [rnd() for _ in range(n_bls)]))
    return RPW(bls[0], bls[1:] + list(ls), list(ns))


def blind_err_witness(n: int, es: Sequence[int], ls: Sequence[int], ns: Sequence[int], rnd: Callable[[], int]) -> RPW:
    """blindErrWitness (:142-149)"""
    bls = pad_right(2 * n + 1, 0, insert_at(n, 0, [rnd() for _ in range(n + 1)]) + list(es))
    return RPW(bls[0], bls[1:] + list(ls), list(ns))


def _scale_errs(n: int, s: int, xs: Sequence[int]) -> List[int]:
    """scaleErrs (:118-121)"""
    xs = list(xs)
    ys, zs = xs[:n + 1], xs[n + 1:]
    a, b = zs[:n - 2], zs[n - 2:]
    return ys + [s * v % N for v in a] + b


def _sum_diagonals(table: Sequence[Sequence[int]]) -> List[int]:
    """sumDiagonals (:104-111)"""
    m: Dict[int, int] = {}
    for a, row in enumerate(table):
        for b, v in enumerate(row):
            m[a + b] = (m.get(a + b, 0) + v) % N
    return [m[k] for k in sorted(m)]


def blind_blinding_term(bl_bls: RPW, tC: int, r0: int, r0_inv: int, r1: int, r1_inv: int, errs: Sequence[int], wits: Sequence[RPW], input_bl: int) -> RPW:
    """blindBlindingTerm (:154-196)"""
    assert bl_bls.sc == 0
    blT, bls_lin, bls_nrm = bl_bls.lin[0], bl_bls.lin[1:], bl_bls.nrm
    rs_inv = r0_inv * r1_inv % N
    n = len(wits)
    wits1, wit_err = wits[:n - 1], wits[n - 1]
    wit_err_row = [wit_err.sc] + pad_right(2 * n, 0, wit_err.lin[:n + 1])
    wit_rows = [[w.sc] + w.lin[:2 * n] for w in wits1]
    wit_rows1 = [[r[0], r[1]] + [(-v) % N for v in r[2:]] for r in wit_rows + [wit_err_row]]
    errs1 = [(-v) % N for v in [(errs[0] - tC * blT) % N] + [rs_inv * v % N for v in errs[1:]]]
    add_consts = lambda a, b, r: [(a * r[0] + b * r[1]) % N] + r[2:]
    table = [insert_at(2 * n - 1, 0, row) for row in
             [errs1] + [_scale_errs(n, r1_inv, add_consts(rs_inv, rs_inv * tC % N, r)) for r in wit_rows1]]
    bl_errs = _scale_errs(n, r1, remove_at(2 * n - 1, _sum_diagonals(table))[:2 * n])
    bl_errs[-1] = (bl_errs[-1] - 2 * input_bl) % N
    return RPW((-bl_errs[0]) % N, [blT] + bl_errs[1:] + list(bls_lin), list(bls_nrm))


# ----------------------------------------------------------------------------- the curve side: backends
class Backend:
    """What the protocol needs from the curve: the Pedersen MSM and the norm-linear argument."""

    def commit(self, scalars: Sequence[int], points: Sequence[Point]) -> Point:
        raise NotImplementedError

    def commit_rows(self, rows: Sequence[Sequence[int]], points: Sequence[Point]) -> List[Point]:
        """one commitment per row of scalars, all over the same points (the input commitments of a proof); default: one MSM each"""
        return [self.commit(r, points) for r in rows]

    def prove_bp(self, flavour: str, n_rounds: int, sc: int, g: Point, q: int, cs, nrm, gs, lin, hs, oracle1: Callable[[List[Point]], int]):
        """proveBPM on PSV(sc, g, makeNormLinearBP q cs nrm gs lin hs) of the NL or IP flavour; returns (responses last round first,
        norm witness, linear witness) = getWitness of the final opening"""
        raise NotImplementedError

    def verify_bp(self, flavour: str, q: int, sp: int, g: Point, pub_nrm, gs, cs, pub_lin, hs, es, responses, wit_nrm, wit_lin, init_terms) -> bool:
        raise NotImplementedError


class GpuBackend(Backend):
    """The product backend: every group operation runs on the MI355X through the C ABI."""

    def __init__(self, gpu):
        self.gpu = gpu

    def commit(self, scalars, points):
        from .capi import points_to_array, scalars_to_array
        if not len(scalars):
            return None
        return self.gpu.msm(scalars_to_array([s % N for s in scalars]), points_to_array(list(points)))

    def commit_rows(self, rows, points):
        """all rows in ONE batched MSM over the shared points (bppp_msm_batch_device, shared_points = 1)"""
        import numpy as np
        from .capi import points_to_array, scalars_to_array
        if not rows:
            return []
        n = len(points)
        d_s = self.gpu.to_device(np.concatenate([scalars_to_array([s % N for s in r]) for r in rows]))
        d_p = self.gpu.to_device(points_to_array(list(points)))
        try:
            return self.gpu.msm_batch_device(d_s, d_p, n, len(rows), shared_points=True)
        finally:
            self.gpu.free(d_s); self.gpu.free(d_p)

    def prove_bp(self, flavour, n_rounds, sc, g, q, cs, nrm, gs, lin, hs, oracle1):
        from .bulletproof import NormLinearBP, NormLinearIP, proveBPM
        com = (NormLinearBP if flavour == "NL" else NormLinearIP)(self.gpu, sc, g, q, cs, nrm, gs, lin, hs)
        try:
            resps, _ = proveBPM(n_rounds, com, oracle1)
            wit = com.getWitness()
        finally:
            com.close()
        return resps, wit[0], wit[1]

    def verify_bp(self, flavour, q, sp, g, pub_nrm, gs, cs, pub_lin, hs, es, responses, wit_nrm, wit_lin, init_terms):
        from .bulletproof import verifyBPM, verifyBPM_IP
        pad = lambda xs, n: list(xs) + [0] * (n - len(xs))
        fn = verifyBPM if flavour == "NL" else verifyBPM_IP
        return fn(self.gpu, q, sp, g, pad(pub_nrm, len(gs)), gs, pad(cs, len(hs)), pad(pub_lin, len(hs)), hs, es, responses, wit_nrm, wit_lin, init_terms)


# ----------------------------------------------------------------------------- transcript (src/ZKP.hs:73-101)
class Transcript:
    """ZKPT's state: all commitments so far (newest first) and the random counter."""

    def __init__(self, oracle: OracleN, rand: Optional[RandFn] = None):
        self.fn, self.rand_fn, self.cs, self.n = oracle, rand, [], 0

    def oracle(self, xs: Sequence[Point], count: int = 1) -> List[int]:
        self.cs = list(xs) + self.cs
        return [v % N for v in self.fn(self.cs, count)]

    def random(self) -> int:
        if self.rand_fn is None:
            raise RuntimeError("No Random in Verifier")        # app/Main.hs:202
        v = self.rand_fn(self.n) % N
        self.n += 1
        return v


def sha256_oracle(tag: bytes = b"") -> OracleN:
    """shaOracle (app/Main.hs:75-80): challenge n = hash (show n <> show (length ps) <> foldMap (coords . toA) ps) with
    coords (A x y) = show x <> show y and hash = decode . SHA-256 — the digest read as a field element by Binary (Prime p)
    (decode_field).  `show` of a field element is taken to be its plain decimal integer (as FastPrime's instance prints it,
    src/Data/Field/Galois/FastPrime.hs:129-130); that text format of the third-party `Prime` type cannot be confirmed offline
    (SURVEY.md 8c), so the hash INPUT is parity-unpinned while the digest decode follows the source.  `tag` (default empty =
    the reference's input) is an optional domain-separation prefix for tests that want distinct oracles.  The native
    counterpart (same bytes in, same challenge out) is csrc/sha256.hip.h + bppp_rp_* (include/bppp.h)."""
    enc: Dict[Point, bytes] = {}

    def one(p: Point) -> bytes:
        b = enc.get(p)
        if b is None:
            b = enc[p] = b"inf" if p is None else str(p[0]).encode() + str(p[1]).encode()
        return b

    def fn(cs: List[Point], count: int) -> List[int]:
        body = b"".join(one(p) for p in cs)
        return [decode_field(hashlib.sha256(tag + str(n).encode() + str(len(cs)).encode() + body).digest(), N) for n in range(1, count + 1)]
    return fn


def hash_to_scalar(prefix: bytes) -> RandFn:
    """hashToScalar rn . show (app/Main.hs:83-84, :189) — the prover's deterministic randomness: hash (prefix <> show n), the
    digest decoded by Binary (Prime p) as everywhere else (decode_field)."""
    return lambda n: decode_field(hashlib.sha256(prefix + str(n).encode()).digest(), N)


# ----------------------------------------------------------------------------- setup (TypedReciprocal.hs:332-359)
@dataclass
class SetupTRRP:
    has_types: bool
    m_bases: List[int]
    sorted_bases: List[int]
    nrm_len: int
    lin_len: int
    pub_vt: List[Tuple[bool, int, int]]
    rds: List[RangeData]
    g: Point
    hs: List[Point]
    gs: List[Point]
    rounds: int
    final_lens: Tuple[int, int]
    backend: Backend
    flavour: str = "NL"

    def base_map(self, x: int) -> Dict[int, int]:
        """makeBaseMap: sortedBases zipped with x^3, x^5, ... (powers'' (x^3) (x^2), :349)"""
        out, c = {}, pow(x, 3, N)
        for b in self.sorted_bases:
            out[b] = c
            c = c * x % N * x % N
        return out

    def q_powers(self, q: int, n: int) -> List[int]:
        """qPowers': powers' (q^2) for the NL Norm (Bulletproof/NormArgument.hs:148), powers' (-q^2) for the IP one
        (Bulletproof/InnerProductArgument.hs:231)"""
        return powers1(q * q % N if self.flavour == "NL" else (-q * q) % N, n)

    def com(self, w: RPW) -> Point:
        """commitRPW sc g lin hs nrm gs (RangeProof/Internal.hs:45-50)"""
        assert len(w.lin) <= len(self.hs) and len(w.nrm) <= len(self.gs)
        return self.backend.commit([w.sc] + list(w.lin) + list(w.nrm), [self.g] + self.hs[:len(w.lin)] + self.gs[:len(w.nrm)])


def round_reduce(n: int) -> int:
    return n // 2 + n % 2


def number_rounds_reduce(n: int) -> Tuple[int, int]:
    """numberRoundsReduce (src/Bulletproof.hs:300-304)"""
    r = 0
    while n >= 5:
        n = round_reduce(n)
        r += 1
    return r, n


def optimal_witness_size(n_len: int, l_len: int, flavour: str = "NL") -> Tuple[int, Tuple[int, int]]:
    """optimalWitnessSize of NormLinear: NL flavour Bulletproof/NormArgument.hs:165-178; IP flavour (the norm vector is paired up
    first and reduced to <= 2 pairs) Bulletproof/InnerProductArgument.hs:253-267 with numberRoundsReduce' (Bulletproof.hs:307-308)"""
    if flavour == "NL":
        nR, n1 = number_rounds_reduce(n_len)
    else:
        nR, n1 = number_rounds_reduce((n_len + n_len % 2) // 2)
        if n1 > 2:
            nR, n1 = nR + 1, round_reduce(n1)
    lR, l1 = number_rounds_reduce(l_len)
    r = max(nR, lR)
    for _ in range(r - nR):
        n1 = round_reduce(n1)
    for _ in range(r - lR):
        l1 = round_reduce(l1)
    w = 1 if flavour == "NL" else 2
    if w * n1 + l1 > 5:
        return r + 1, (w * round_reduce(n1), round_reduce(l1))
    return r, (w * n1, l1)


def setup(backend: Backend, points: Sequence[Point], has_types: bool, pub_vt: Sequence[Tuple[bool, int, int]], rds: Sequence[RangeData],
          flavour: str = "NL") -> SetupTRRP:
    """setup (TypedReciprocal.hs:332-359): points = h : g : ps (h is not used by the proof, as in the reference)."""
    live = [rd for rd in rds if not rd.is_assumed]
    any_has_bit = any(rd.has_bit for rd in live)
    any_shared_has_bit = any(rd.has_bit and rd.is_shared for rd in live)
    pairs = sorted(((rd.is_shared, rd.base) for rd in live), key=lambda p: p[1])
    m_bases = sorted(set(([2] if any_shared_has_bit else []) + [b for s, b in pairs if s]))
    sorted_bases = sorted(set(([2] if any_has_bit else []) + [b for _, b in pairs]))
    nrm_len = sum(len(rd.base_coeffs) + (1 if has_types else 0) for rd in rds)
    lin_len = 6 + sum(b - 1 for b in m_bases)
    ps = list(points[2:])
    if len(ps) < lin_len + nrm_len:
        raise ValueError("not enough basis points")
    if flavour not in ("NL", "IP"):
        raise ValueError("argument flavour must be NL or IP")
    rounds, final = optimal_witness_size(nrm_len, lin_len, flavour)
    return SetupTRRP(has_types, m_bases, sorted_bases, nrm_len, lin_len, list(pub_vt), list(rds), points[1], ps[:lin_len], ps[lin_len:lin_len + nrm_len],
                     rounds, final, backend, flavour)


# ----------------------------------------------------------------------------- witness (TypedReciprocal.hs:361-389)
@dataclass
class WitnessTRRP:
    inputs: List[Tuple[int, int, int]]       # (amount, type, blinding) per input — the PedersenScalarPair's scalars
    ph1s: list
    base_mss: List[Tuple[int, List[int]]]


def witness(st: SetupTRRP, inputs: Sequence[Tuple[int, int, int]]) -> WitnessTRRP:
    """witnessTRRP (:372-389): inputs are (amount, type, blinding)."""
    if len(inputs) != len(st.rds):
        raise ValueError("Different number of values and ranges")
    if st.has_types:
        sums: Dict[int, int] = {}
        for io, ty, v in st.pub_vt:
            sums[ty % N] = (sums.get(ty % N, 0) + (-v if io else v)) % N
        for (v, ty, _), rd in zip(inputs, st.rds):
            sums[ty % N] = (sums.get(ty % N, 0) + (-v if rd.is_output else v)) % N
        if any(sums.values()):
            raise ValueError("amounts of some type do not balance")
    ph1ss, mss = [], []
    for i, ((v, _, _), rd) in enumerate(zip(inputs, st.rds)):
        p, m = make_phase1s(i, rd, v)
        ph1ss.append(p); mss.append(m)
    types = [("typing", i, rd.is_output, rd.is_assumed, v % N, ty % N) for i, ((v, ty, _), rd) in enumerate(zip(inputs, st.rds))]
    ph1s = (types if st.has_types else []) + [p for ps_ in ph1ss for p in ps_]
    acc: Dict[int, List[int]] = {}
    add = lambda b, ms: acc.__setitem__(b, [(x + y) % N for x, y in zip(acc[b], ms)] if b in acc else list(ms))
    for rd, ms in zip(st.rds, mss):                      # baseMss (:363-370)
        if ms is None:
            continue
        if rd.has_bit:
            add(2, [ms[0]]); add(rd.base, ms[1:])
        else:
            add(rd.base, ms)
    return WitnessTRRP([(v % N, ty % N, bl % N) for v, ty, bl in inputs], ph1s, sorted(acc.items()))


# ----------------------------------------------------------------------------- proof object and the two protocol halves
@dataclass
class RangeProof:
    """RP coms (PBP responses opening) (src/RangeProof.hs:90): coms = blCom : rCom : dmCom : mCom : nComs."""
    coms: List[Point]
    responses: List[Tuple[Point, Point]]      # last round first
    wit_nrm: List[int]
    wit_lin: List[int]


@dataclass
class SetupBP:
    """SBP basis initCom publicCs rounds (src/Bulletproof.hs:327-328), flattened to what verifyBPM consumes."""
    q: int
    cs: List[int]
    pub: RPW
    init_terms: List[Tuple[int, Point]]
    rounds: int


def _init_terms(st: SetupTRRP, coms: Sequence[Point], x: int, q0: int, t: int) -> List[Tuple[int, Point]]:
    """openWith of TranscriptTRRP (TypedReciprocal.hs:293-297)"""
    bl, r, dm, m = coms[:4]
    tp = lambda k: pow(t, k, N)
    ss = [2 * tp(5) * c % N for c in input_coeffs(st.has_types, [rd.is_assumed for rd in st.rds], x, q0)]
    return list(zip(ss, coms[4:])) + [(1, bl), (t % N, m), (tp(2), dm), (tp(3), r)]


def prove_rp(st: SetupTRRP, w: WitnessTRRP, tr: Transcript) -> Tuple[List[Point], SetupBP, RPW]:
    """proveTRRPM (TypedReciprocal.hs:399-446)"""
    num_terms = 3
    is_as = [rd.is_assumed for rd in st.rds]
    m_bases = [b for b, _ in w.base_mss]
    if m_bases != st.m_bases:
        raise ValueError("witness does not cover the setup's shared bases")
    ms_shared = [m for _, ms in w.base_mss for m in ms]
    ds, ms_inline = get_ds_ms(w.ph1s)

    n_wits = [RPW(v, [ty, bl], []) for v, ty, bl in w.inputs]                    # scalarPairRPW' (Internal.hs:59-60)
    n_coms = st.backend.commit_rows([[nw.sc] + nw.lin for nw in n_wits], [st.g] + st.hs[:2])   # = [st.com(nw) ...], one launch
    dm_wit = blind_witness(num_terms, 2, ms_shared, ds, tr.random); dm_com = st.com(dm_wit)
    m_wit = blind_witness(num_terms, 1, [], ms_inline, tr.random); m_com = st.com(m_wit)

    e, x, r0 = tr.oracle([dm_com, m_com] + n_coms, 3)
    e_inv, r0_inv = batch_inverse([e, r0])

    base_map = st.base_map(x)
    ph2s = make_phase2s(e, e_inv, x, base_map, w.ph1s, private=True)
    err7 = r0_inv * (-sum(2 * p.r * p.c for p in ph2s)) % N                      # err7Term (:209-211)
    r_wit = blind_err_witness(num_terms, [err7], [], [p.r for p in ph2s], tr.random); r_com = st.com(r_wit)

    q, xp, r1 = tr.oracle([r_com], 3)
    q0 = st.q_powers(q, 1)[0]
    q_inv, q0_inv, r1_inv = batch_inverse([q, q0, r1])
    shared_cs = make_shared_coeffs(e, e_inv, m_bases, base_map)
    tC = xp if st.has_types else 0

    bls_lin = [tr.random() for _ in range(st.lin_len - 5)]
    bls_nrm = [tr.random() for _ in range(st.nrm_len)]
    bls_ms = bls_lin[1:]

    n_wit_sum = RPW()
    for c, nw in zip(input_coeffs(st.has_types, is_as, x, q0), n_wits):
        n_wit_sum = n_wit_sum + nw.scale(c)
    input_bl = n_wit_sum.lin[1]
    ph3s = list(zip(ph2s, st.q_powers(q, len(ph2s)), bls_nrm))                  # the q^-2i of Ph3 are not used by makeErrorTerms
    errs = make_error_terms(e, xp, shared_cs, bls_ms, ph3s)
    bl_wit = blind_blinding_term(RPW(0, bls_lin, bls_nrm), tC, r0, r0_inv, r1, r1_inv, errs, [m_wit, dm_wit, r_wit], input_bl)
    bl_com = st.com(bl_wit)
    t = tr.oracle([bl_com], 1)[0]

    pub = make_public_consts(e, e_inv, x, xp, q0, q0_inv, t, st.has_types, st.rds, st.pub_vt, ph2s)
    tp = lambda k: pow(t, k, N)
    wit = pub + bl_wit + m_wit.scale(t) + dm_wit.scale(tp(2)) + r_wit.scale(tp(3)) + n_wit_sum.scale(2 * tp(5) % N)
    coms = [bl_com, r_com, dm_com, m_com] + n_coms
    cs = make_bp_coeffs(st.has_types, xp, r0, r1, t, shared_cs)
    return coms, SetupBP(q, cs, pub, _init_terms(st, coms, x, q0, t), st.rounds), wit


def verify_rp(st: SetupTRRP, coms: Sequence[Point], tr: Transcript) -> SetupBP:
    """verifyTRRPM (TypedReciprocal.hs:449-467)"""
    if len(coms) != 4 + len(st.rds):
        raise ValueError("wrong number of range-proof commitments")
    ph1ss = [make_phase1s(i, rd, None)[0] for i, rd in enumerate(st.rds)]
    types = [("typing", i, rd.is_output, rd.is_assumed, None, None) for i, rd in enumerate(st.rds)]
    ph1s = (types if st.has_types else []) + [p for ps_ in ph1ss for p in ps_]
    bl_com, r_com, dm_com, m_com = coms[:4]
    e, x, r0 = tr.oracle([dm_com, m_com] + list(coms[4:]), 3)
    q, xp, r1 = tr.oracle([r_com], 3)
    q0 = st.q_powers(q, 1)[0]
    t = tr.oracle([bl_com], 1)[0]
    e_inv, _, q0_inv = batch_inverse([e, q, q0])
    base_map = st.base_map(x)
    ph2s = make_phase2s(e, e_inv, x, base_map, ph1s, private=False)
    pub = make_public_consts(e, e_inv, x, xp, q0, q0_inv, t, st.has_types, st.rds, st.pub_vt, ph2s)
    cs = make_bp_coeffs(st.has_types, xp, r0, r1, t, make_shared_coeffs(e, e_inv, st.m_bases, base_map))
    return SetupBP(q, cs, pub, _init_terms(st, coms, x, q0, t), st.rounds)


# ----------------------------------------------------------------------------- ZKP instance of RangeProof (src/RangeProof.hs:93-105)
def prove(st: SetupTRRP, w: WitnessTRRP, oracle: OracleN, rand: RandFn) -> RangeProof:
    """proveM: proveRP, then the norm-linear argument on the combined witness (proveBPM, src/Bulletproof.hs:357-359)."""
    tr = Transcript(oracle, rand)
    coms, sbp, wit = prove_rp(st, w, tr)
    resps, nw, lw = st.backend.prove_bp(st.flavour, sbp.rounds, wit.sc, st.g, sbp.q, sbp.cs, wit.nrm, st.gs, wit.lin, st.hs, lambda xs: tr.oracle(xs, 1)[0])
    return RangeProof(coms, resps, nw, lw)


def verify_inputs(st: SetupTRRP, proof: RangeProof, oracle: OracleN) -> Optional[dict]:
    """verifyRP plus the challenge derivation of verifyBPM (src/Bulletproof.hs:374): everything the (batch) verifier's MSM needs.
    None if the proof is malformed (wrong lengths)."""
    if len(proof.responses) != st.rounds or (len(proof.wit_nrm), len(proof.wit_lin)) != st.final_lens or len(proof.coms) != 4 + len(st.rds):
        return None
    tr = Transcript(oracle)
    sbp = verify_rp(st, proof.coms, tr)
    es: List[int] = []
    for a, b in reversed(proof.responses):            # foldrM: first round first, consed => last round first
        es.insert(0, tr.oracle([a, b], 1)[0])
    pad = lambda xs, n: list(xs) + [0] * (n - len(xs))
    return {"q": sbp.q, "sp": sbp.pub.sc, "pub_norm": pad(sbp.pub.nrm, st.nrm_len), "pub_lin_c": pad(sbp.cs, st.lin_len), "pub_lin_x": pad(sbp.pub.lin, st.lin_len),
            "es": es, "responses": list(proof.responses), "wit_norm": list(proof.wit_nrm), "wit_lin": list(proof.wit_lin), "init_terms": sbp.init_terms}


def verify(st: SetupTRRP, proof: RangeProof, oracle: OracleN) -> bool:
    """verifyM (src/RangeProof.hs:103-105; src/Bulletproof.hs:343, :370-378)"""
    v = verify_inputs(st, proof, oracle)
    if v is None:
        return False
    return st.backend.verify_bp(st.flavour, v["q"], v["sp"], st.g, v["pub_norm"], st.gs, v["pub_lin_c"], v["pub_lin_x"], st.hs, v["es"], v["responses"], v["wit_norm"],
                                v["wit_lin"], v["init_terms"])


# ----------------------------------------------------------------------------- device-side verifier scalars (csrc/trrp.hip)
def verifier_challenges(st: SetupTRRP, proof: RangeProof, oracle: OracleN) -> Optional[Tuple[List[int], List[int]]]:
    """The oracle calls of verifyTRRPM (TypedReciprocal.hs:459-462) and of verifyBPM (Bulletproof.hs:374), nothing else:
    ((e, x, r0, q, x', r1, t), [e_k ... e_1])  — the host's whole share of a device-derived verification."""
    if len(proof.responses) != st.rounds or (len(proof.wit_nrm), len(proof.wit_lin)) != st.final_lens or len(proof.coms) != 4 + len(st.rds):
        return None
    tr = Transcript(oracle)
    bl_com, r_com, dm_com, m_com = proof.coms[:4]
    e, x, r0 = tr.oracle([dm_com, m_com] + list(proof.coms[4:]), 3)
    q, xp, r1 = tr.oracle([r_com], 3)
    t = tr.oracle([bl_com], 1)[0]
    es: List[int] = []
    for a, b in reversed(proof.responses):
        es.insert(0, tr.oracle([a, b], 1)[0])
    return [e, x, r0, q, xp, r1, t], es


class DeviceVerifierTables:
    """The static structure of one setup uploaded for bppp_trrp_public_device: from then on a proof's public scalars
    (makePublicConsts, makeBpCoeffs, the initCom scalars) are computed on the GPU from its seven challenges."""

    def __init__(self, gpu, st: SetupTRRP):
        import ctypes as C
        import numpy as np
        from .capi import _ptr, scalars_to_array
        self.gpu, self.st, self.h = gpu, st, None
        ph1ss = [make_phase1s(i, rd, None)[0] for i, rd in enumerate(st.rds)]
        types = [("typing", i, rd.is_output, rd.is_assumed, None, None) for i, rd in enumerate(st.rds)]
        ph1s = (types if st.has_types else []) + [p for ps_ in ph1ss for p in ps_]
        if len(ph1s) != st.nrm_len:
            raise ValueError("phase-1 layout does not match the setup's norm length")
        slot_of = {b: k for k, b in enumerate(st.sorted_bases)}
        syms: List[int] = []
        sym_idx: Dict[int, int] = {}

        def sym(v: int) -> int:
            v %= N
            if v not in sym_idx:
                sym_idx[v] = len(syms)
                syms.append(v)
            return sym_idx[v]
        kind, rng_, slot, psym, coeff = [], [], [], [], []
        for p in ph1s:
            if p[0] == "typing":
                kind.append(0 | (0x100 if p[2] else 0) | (0x200 if p[3] else 0)); rng_.append(p[1]); slot.append(0); psym.append(0xFFFFFFFF); coeff.append(0)
            elif p[0] == "inline":
                kind.append(1); rng_.append(p[1]); slot.append(slot_of[p[2]]); psym.append(sym(p[6]) if p[6] else 0xFFFFFFFF); coeff.append(p[3])
            else:
                kind.append(2); rng_.append(p[1]); slot.append(slot_of[p[2]]); psym.append(0xFFFFFFFF); coeff.append(p[3])
        cs_slot, cs_sym = [], []
        for b in st.m_bases:
            for s_ in range(1, b):
                cs_slot.append(slot_of[b]); cs_sym.append(sym(s_))
        if 6 + len(cs_slot) != st.lin_len:
            raise ValueError("shared-base layout does not match the setup's linear length")
        pub_out = [1 if io else 0 for io, _, _ in st.pub_vt]
        pub_sym = [sym(ty) for _, ty, _ in st.pub_vt]
        pub_amt = [v % N for _, _, v in st.pub_vt]
        u32 = lambda xs: np.ascontiguousarray(np.array(list(xs) or [0], dtype=np.uint32))
        sc = lambda xs: scalars_to_array(list(xs) or [0])
        self._keep = [u32(kind), u32(rng_), u32(slot), u32(psym), sc(coeff), sc([rd.lo % N for rd in st.rds]), u32([1 if rd.is_assumed else 0 for rd in st.rds]),
                      sc(syms), u32(cs_slot), u32(cs_sym), u32(pub_out), sc(pub_amt), u32(pub_sym)]
        k = self._keep
        h = C.c_void_p()
        rc = gpu.lib.bppp_trrp_create(gpu.h, 0 if st.flavour == "NL" else 1, int(st.has_types), st.nrm_len, st.lin_len, len(st.rds), _ptr(k[0]), _ptr(k[1]), _ptr(k[2]),
                                      _ptr(k[3]), _ptr(k[4]), _ptr(k[5]), _ptr(k[6]), len(syms), _ptr(k[7]), _ptr(k[8]), _ptr(k[9]), len(st.pub_vt), _ptr(k[10]),
                                      _ptr(k[11]), _ptr(k[12]), C.byref(h))
        gpu._check(rc, "bppp_trrp_create")
        self.h = h
        gpu._adopt(self)
        self.ninit = 4 + len(st.rds)

    def close(self):
        if self.h:
            self.gpu.lib.bppp_trrp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def public_device(self, batch: int, d_challenges: int, d_q: int, d_sp: int, d_pub_norm: int, d_pub_lin_c: int, d_init_scalars: int):
        """device pointers in, device arrays out (see include/bppp.h); the arrays are complete on return"""
        from .capi import _ptr
        self.gpu._check(self.gpu.lib.bppp_trrp_public_device(self.h, batch, _ptr(d_challenges), _ptr(d_q), _ptr(d_sp), _ptr(d_pub_norm), _ptr(d_pub_lin_c),
                                                             _ptr(d_init_scalars)), "bppp_trrp_public_device")

    def public(self, challenges: Sequence[Sequence[int]]) -> List[dict]:
        """host convenience (tests): the derived scalars of each proof as Python integers"""
        import numpy as np
        from .capi import array_to_scalars, scalars_to_array
        B, st, gpu = len(challenges), self.st, self.gpu
        d_ch = gpu.to_device(np.concatenate([scalars_to_array([c % N for c in ch]) for ch in challenges]))
        sizes = {"q": B, "sp": B, "pn": B * st.nrm_len, "cs": B * st.lin_len, "init": B * self.ninit}
        bufs = {k: gpu.to_device(np.zeros((n, 4), dtype=np.uint64)) for k, n in sizes.items()}
        try:
            self.public_device(B, d_ch, bufs["q"], bufs["sp"], bufs["pn"], bufs["cs"], bufs["init"])
            host = {k: array_to_scalars(gpu.download(bufs[k], (n, 4))) for k, n in sizes.items()}
        finally:
            gpu.free(d_ch)
            for p in bufs.values():
                gpu.free(p)
        cut = lambda xs, n, b: xs[b * n:(b + 1) * n]
        return [{"q": host["q"][b], "sp": host["sp"][b], "pub_norm": cut(host["pn"], st.nrm_len, b), "pub_lin_c": cut(host["cs"], st.lin_len, b),
                 "init_scalars": cut(host["init"], self.ninit, b)} for b in range(B)]


# ----------------------------------------------------------------------------- the native range-proof layer (csrc/rp.hip)
class NativeRangeProofs:
    """One setup registered with the library (bppp_rp_create): ranges, layout and basis live on the device; batches of ENCODED
    proofs (the reference's commitments / proof files, bulletproofspp_amd.encoding) are verified end to end there — decoding,
    all SHA-256 transcript hashing (the CLI's shaOracle), verifyTRRPM's scalars, challenge expansion and one combined MSM.
    Both argument flavours verify and prove (bppp_rp_prove_batch: the norm-linear argument through csrc/nlb.hip, the inner-product one
    through csrc/ipb.hip once the handle has its comb table, csrc/rpprove.hip's host-algebra ip_argument_lockstep before that)."""

    def __init__(self, gpu, st: SetupTRRP, oracle_tag: bytes = b"", h: Point = None, basis_seed: Optional[bytes] = None):
        """basis_seed: the schema's "basisSeed" as bytes — the library derives the basis from it on the GPU (bppp_rp_create_seeded:
        getPoints from candidate 0) instead of taking st's points; `st` must be the setup over that same stream (setup_from_schema)."""
        import ctypes as C
        from .capi import RP_ASSUMED, RP_OUTPUT, RP_SHARED, RpPublic, RpRange, RpShape, int_to_limbs, points_to_array
        self.gpu, self.st, self.h = gpu, st, None
        rng = (RpRange * len(st.rds))()
        for r, rd in zip(rng, st.rds):
            r.base = rd.base
            r.flags = (RP_SHARED if rd.is_shared else 0) | (RP_OUTPUT if rd.is_output else 0) | (RP_ASSUMED if rd.is_assumed else 0)
            r.min[:] = [int(v) for v in int_to_limbs(rd.lo % 2**256)]     # two's complement: a minimum may be negative (examples/rec_test)
            r.max[:] = [int(v) for v in int_to_limbs(rd.hi % 2**256)]
        pubs = (RpPublic * max(len(st.pub_vt), 1))()
        for p_, (io, ty, v) in zip(pubs, st.pub_vt):
            p_.is_output = 1 if io else 0
            p_.type[:] = [int(x) for x in int_to_limbs(ty % N)]
            p_.amount[:] = [int(x) for x in int_to_limbs(v % N)]
        hnd = C.c_void_p()
        if basis_seed is not None:
            rc = gpu.lib.bppp_rp_create_seeded(gpu.h, 0 if st.flavour == "NL" else 1, int(st.has_types), C.cast(rng, C.c_void_p), len(st.rds), C.cast(pubs, C.c_void_p),
                                               len(st.pub_vt), bytes(basis_seed), len(basis_seed), oracle_tag if oracle_tag else None, C.byref(hnd))
            gpu._check(rc, "bppp_rp_create_seeded")
        else:
            pts = points_to_array([h if h is not None else st.g, st.g] + list(st.hs) + list(st.gs))
            rc = gpu.lib.bppp_rp_create(gpu.h, 0 if st.flavour == "NL" else 1, int(st.has_types), C.cast(rng, C.c_void_p), len(st.rds), C.cast(pubs, C.c_void_p), len(st.pub_vt),
                                        C.c_void_p(pts.ctypes.data), pts.shape[0], oracle_tag if oracle_tag else None, C.byref(hnd))
            gpu._check(rc, "bppp_rp_create")
        self.h = hnd
        gpu._adopt(self)
        shp = RpShape()
        gpu._check(gpu.lib.bppp_rp_info(self.h, C.byref(shp)), "bppp_rp_info")
        self.shape = {n: int(getattr(shp, n)) for n, _ in RpShape._fields_}
        if (self.shape["norm_len"], self.shape["lin_len"], self.shape["rounds"], (self.shape["final_norm"], self.shape["final_lin"])) != \
                (st.nrm_len, st.lin_len, st.rounds, tuple(st.final_lens)):
            raise RuntimeError("native setup disagrees with the host setup: %r" % (self.shape,))

    def close(self):
        if self.h:
            self.gpu.lib.bppp_rp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name: str, value: int):
        """bppp_rp_set_option: comb_min, comb_budget, comb_bits, split_min, host_oracle_max, fold_points, host_algebra, timing, culprits"""
        from .capi import RP_OPTIONS
        self.gpu._check(self.gpu.lib.bppp_rp_set_option(self.h, RP_OPTIONS[name], int(value)), "bppp_rp_set_option")

    def public_count(self) -> int:
        """bppp_rp_public_count: public amounts per proof the *_pub calls take (npub of a typed handle, 1 of a conserved binary one, else 0)"""
        import ctypes as C
        n = C.c_size_t(0)
        self.gpu._check(self.gpu.lib.bppp_rp_public_count(self.h, C.byref(n)), "bppp_rp_public_count")
        return int(n.value)

    def _public_words(self, public_amounts, B: int):
        """B per-proof public amount lists -> [B * npub][4] words of canonical scalars (reduced mod N, as the constructor does for pub_vt)"""
        from .capi import scalars_to_array
        if len(public_amounts) != B:
            raise ValueError("one list of public amounts per proof is required")
        return scalars_to_array([int(v) % N for row in public_amounts for v in row] or [0])

    @contextlib.contextmanager
    def _public_arg(self, public_amounts, B: int, device: bool):
        """the *_pub entry points' amounts argument: NULL for None (include/bppp.h: exactly the call without _pub), a device pointer (int)
        as given, else per-proof values — uploaded for a device entry point, the copy freed after the call"""
        import ctypes as C
        if public_amounts is None or isinstance(public_amounts, int):
            yield C.c_void_p(public_amounts)
            return
        words = self._public_words(public_amounts, B)
        if not device:
            yield C.c_void_p(words.ctypes.data)
            return
        d = self.gpu.to_device(words)
        try:
            yield C.c_void_p(d)
        finally:
            self.gpu.free(d)

    @contextlib.contextmanager
    def _bindings_arg(self, bindings, B: int, device: bool):
        """the *_bound entry points' bindings argument: per-proof 32-byte values (capi.bindings_array: a sequence of bytes or a [B, 32] uint8
        array; ValueError for anything else, before any library call) — uploaded for a device entry point, the copy freed after the call — or,
        for a device entry point, a device pointer (int) to the [B][32] bytes as given"""
        import ctypes as C
        from .capi import bindings_array
        if device and isinstance(bindings, int):
            yield C.c_void_p(bindings)
            return
        arr = bindings_array(bindings, B)
        if not device:
            yield C.c_void_p(arr.ctypes.data)
            return
        d = self.gpu.to_device(arr)
        try:
            yield C.c_void_p(d)
        finally:
            self.gpu.free(d)

    def prove_batch(self, inputs: Sequence[Sequence[Tuple[int, int, int]]], rand_prefixes: Sequence[bytes], public_amounts=None, bindings=None) -> List[Tuple[bytes, bytes]]:
        """bppp_rp_prove_batch: inputs[b] = [(amount, type, blinding) per range]; rand_prefixes[b] = the hashToScalar prefix of
        proof b (all of one length).  Returns [(commitments file, proof file)] — the bytes encoding.encode_proof(prove(...)) gives.
        public_amounts (bppp_rp_prove_batch_pub): per proof, the public amounts that replace the setup's (one list per proof on a typed
        handle, in pub_vt's order; one int per proof on a binary one); None = the setup's.
        bindings (bppp_rp_prove_bound): per proof, 32 bytes that tie the proof to its transaction — proof b is the proof of a handle whose
        oracle tag is tag + bindings[b]; None = the unbound call."""
        import ctypes as C
        from .capi import bindings_array
        B = len(inputs)
        bindings_array(bindings, B)
        if B == 0:
            return []
        amt, typ, bld, pre, plen, cf, pf = self._prove_arrays(inputs, rand_prefixes)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        with self._public_arg(public_amounts, B, False) as pa:
            if bindings is None:
                rc = self.gpu.lib.bppp_rp_prove_batch_pub(self.h, B, vp(amt), vp(typ), vp(bld), pa, vp(pre), plen, vp(cf), vp(pf))
            else:
                with self._bindings_arg(bindings, B, False) as ba:
                    rc = self.gpu.lib.bppp_rp_prove_bound(self.h, B, vp(amt), vp(typ), vp(bld), pa, ba, vp(pre), plen, vp(cf), vp(pf), None)
        self.gpu._check(rc, "bppp_rp_prove_batch" if bindings is None else "bppp_rp_prove_bound")
        return self._prove_files(B, cf, pf)

    def prove_batch_device(self, batch: int, d_amounts: int, d_types: int, d_blinds: int, d_prefix: int, prefix_len: int, d_coms: int, d_proofs: int,
                           d_public_amounts: int = 0, bindings=None):
        """bppp_rp_prove_batch_device: prove_batch with every buffer in HBM (device pointers, the layouts of _prove_arrays; d_types is 0 on a
        binary handle, d_public_amounts 0 = the setup's amounts).  On return d_coms / d_proofs hold the files prove_batch returns.
        bindings (bppp_rp_prove_bound_device): as for prove_batch (uploaded for the call), or a device pointer to the [batch][32] bytes."""
        import ctypes as C
        if bindings is None:
            self.gpu.rp_prove_batch_device(self.h, batch, d_amounts, d_types, d_blinds, d_public_amounts, d_prefix, prefix_len, d_coms, d_proofs)
            return
        p = lambda v: C.c_void_p(v or None)
        with self._bindings_arg(bindings, batch, True) as ba:
            rc = self.gpu.lib.bppp_rp_prove_bound_device(self.h, batch, p(d_amounts), p(d_types), p(d_blinds), p(d_public_amounts), ba, p(d_prefix), prefix_len, p(d_coms),
                                                         p(d_proofs), None)
        self.gpu._check(rc, "bppp_rp_prove_bound_device")

    def prove_batch_status(self, inputs, rand_prefixes: Sequence[bytes], public_amounts=None, bindings=None):
        """bppp_rp_prove_batch_status: prove_batch that refuses proof by proof.  Returns (files, statuses): files[b] is (commitments file, proof
        file) — the bytes prove_batch gives for proof b alone — or None for a refused proof; statuses[b] is its capi.RP_WIT_* verdict (0 =
        accepted).  bindings as for prove_batch (bppp_rp_prove_bound with proof_status)."""
        import ctypes as C
        import numpy as np
        from .capi import bindings_array
        B = len(inputs)
        bindings_array(bindings, B)
        if B == 0:
            return [], []
        amt, typ, bld, pre, plen, cf, pf = self._prove_arrays(self._prove_rows(inputs), rand_prefixes)
        status = np.zeros(B, dtype=np.uint32)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        with self._public_arg(public_amounts, B, False) as pa:
            if bindings is None:
                rc = self.gpu.lib.bppp_rp_prove_batch_status(self.h, B, vp(amt), vp(typ), vp(bld), pa, vp(pre), plen, vp(cf), vp(pf), vp(status))
            else:
                with self._bindings_arg(bindings, B, False) as ba:
                    rc = self.gpu.lib.bppp_rp_prove_bound(self.h, B, vp(amt), vp(typ), vp(bld), pa, ba, vp(pre), plen, vp(cf), vp(pf), vp(status))
        self.gpu._check(rc, "bppp_rp_prove_batch_status" if bindings is None else "bppp_rp_prove_bound")
        files = self._prove_files(B, cf, pf)
        return [f if s == 0 else None for f, s in zip(files, status)], [int(s) for s in status]

    def prove_batch_status_device(self, batch: int, d_amounts: int, d_types: int, d_blinds: int, d_prefix: int, prefix_len: int, d_coms: int, d_proofs: int,
                                  d_public_amounts: int = 0, bindings=None):
        """bppp_rp_prove_batch_status_device: prove_batch_device that refuses proof by proof.  Returns the verdicts (numpy uint32 [batch], capi.RP_WIT_*); on
        return d_coms / d_proofs hold the accepted proofs' files and zero bytes for the refused ones.  bindings as for prove_batch_device
        (bppp_rp_prove_bound_device with proof_status)."""
        import ctypes as C
        import numpy as np
        if bindings is None:
            return self.gpu.rp_prove_batch_status_device(self.h, batch, d_amounts, d_types, d_blinds, d_public_amounts, d_prefix, prefix_len, d_coms, d_proofs)
        status = np.zeros(max(batch, 1), dtype=np.uint32)
        p = lambda v: C.c_void_p(v or None)
        with self._bindings_arg(bindings, batch, True) as ba:
            rc = self.gpu.lib.bppp_rp_prove_bound_device(self.h, batch, p(d_amounts), p(d_types), p(d_blinds), p(d_public_amounts), ba, p(d_prefix), prefix_len, p(d_coms),
                                                         p(d_proofs), C.c_void_p(status.ctypes.data))
        self.gpu._check(rc, "bppp_rp_prove_bound_device")
        return status[:batch]

    def _prove_rows(self, inputs):
        """one (amount, type, blinding) per range, as this class's prove_batch takes its inputs"""
        return inputs

    def _prove_arrays(self, inputs, rand_prefixes):
        """the prove entry points' arrays for `inputs` [(amount, type, blinding) per range] per proof: amounts, types, blindings, prefixes,
        the prefix length and the two zeroed output buffers"""
        import numpy as np
        from .capi import scalars_to_array
        B, nr = len(inputs), len(self.st.rds)
        if len(rand_prefixes) != B or len({len(p_) for p_ in rand_prefixes}) != 1 or any(len(row) != nr for row in inputs):
            raise ValueError("one equal-length randomness prefix per proof and one (amount, type, blinding) per range are required")
        amt = scalars_to_array([v % 2**256 for row in inputs for v, _, _ in row])
        typ = scalars_to_array([t % N for row in inputs for _, t, _ in row])
        bld = scalars_to_array([b_ % N for row in inputs for _, _, b_ in row])
        pre = np.frombuffer(b"".join(rand_prefixes) or b"\0", dtype=np.uint8)
        cf = np.zeros(B * self.shape["coms_bytes"], dtype=np.uint8)
        pf = np.zeros(B * self.shape["proof_bytes"], dtype=np.uint8)
        return amt, typ, bld, pre, len(rand_prefixes[0]), cf, pf

    def _prove_files(self, B, cf, pf):
        cb, pb = self.shape["coms_bytes"], self.shape["proof_bytes"]
        return [(cf[b * cb:(b + 1) * cb].tobytes(), pf[b * pb:(b + 1) * pb].tobytes()) for b in range(B)]

    # ---- commitments without a proof, and their openings (bppp_rp_commit_batch / bppp_rp_open_each / bppp_rp_open_batch)
    def _claim_arrays(self, inputs):
        """amounts, types, blindings of `inputs` (the shape prove_batch takes) as the entry points' [B * nranges][4] word arrays"""
        from .capi import scalars_to_array
        rows, nr = self._prove_rows(inputs), len(self.st.rds)
        if any(len(row) != nr for row in rows):
            raise ValueError("one (amount, type, blinding) per range is required")
        return (scalars_to_array([v % 2**256 for row in rows for v, _, _ in row] or [0]), scalars_to_array([t for row in rows for _, t, _ in row] or [0]),
                scalars_to_array([b_ for row in rows for _, _, b_ in row] or [0]))

    def _coms_array(self, coms_files, B):
        import numpy as np
        if len(coms_files) != B or any(len(c) != self.shape["coms_bytes"] for c in coms_files):
            raise ValueError("one commitments file of coms_bytes per row of inputs is required")
        return np.frombuffer(b"".join(coms_files) or b"\0", dtype=np.uint8)

    def commit_batch(self, inputs, want_status: bool = False):
        """bppp_rp_commit_batch: the commitments file of every row of `inputs` (prove_batch's shape; types and blindings are passed as given,
        so a value >= N is the library's to refuse) — no witness is judged.  Returns the files, or (files, statuses) with want_status: a refused
        row (capi.RP_WIT_NOT_CANONICAL / RP_WIT_BIN_NOT_CANONICAL / RP_COMMIT_INFINITY) has None for its file.  Without want_status a refused
        row raises BpppError."""
        import ctypes as C
        import numpy as np
        B, cb = len(inputs), self.shape["coms_bytes"]
        if B == 0:
            return ([], []) if want_status else []
        amt, typ, bld = self._claim_arrays(inputs)
        cf, status = np.zeros(B * cb, dtype=np.uint8), np.zeros(B, dtype=np.uint32)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        rc = self.gpu.lib.bppp_rp_commit_batch(self.h, B, vp(amt), vp(typ), vp(bld), vp(status) if want_status else None, vp(cf))
        self.gpu._check(rc, "bppp_rp_commit_batch")
        files = [cf[b * cb:(b + 1) * cb].tobytes() for b in range(B)]
        return ([f if s == 0 else None for f, s in zip(files, status)], [int(s) for s in status]) if want_status else files

    def commit_batch_device(self, batch: int, d_amounts: int, d_types: int, d_blinds: int, d_coms: int, want_status: bool = False):
        """bppp_rp_commit_batch_device: commit_batch with every buffer in HBM (device pointers; d_types is 0 on a binary handle).  On return
        d_coms holds the files; returns the verdicts (numpy uint32 [batch]) with want_status, else None (a refused row raises)."""
        import ctypes as C
        import numpy as np
        status = np.zeros(max(batch, 1), dtype=np.uint32)
        rc = self.gpu.lib.bppp_rp_commit_batch_device(self.h, batch, C.c_void_p(d_amounts), C.c_void_p(d_types), C.c_void_p(d_blinds),
                                                      C.c_void_p(status.ctypes.data) if want_status else None, C.c_void_p(d_coms))
        self.gpu._check(rc, "bppp_rp_commit_batch_device")
        return status[:batch] if want_status else None

    def open_each(self, coms_files: Sequence[bytes], inputs):
        """bppp_rp_open_each: does commitment i of file b open to inputs[b][i]?  Returns [batch][nranges] ints (capi.RP_OPEN_*): exact, no weights."""
        import ctypes as C
        B = len(inputs)
        if B == 0:
            return []
        amt, typ, bld = self._claim_arrays(inputs)
        cf = self._coms_array(coms_files, B)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        return self._open_each(self.gpu.lib.bppp_rp_open_each, B, vp(cf), vp(amt), vp(typ), vp(bld))

    def open_each_device(self, batch: int, d_coms: int, d_amounts: int, d_types: int, d_blinds: int):
        """bppp_rp_open_each_device: open_each on buffers already in HBM (device pointers; d_types is 0 on a binary handle)"""
        import ctypes as C
        return self._open_each(self.gpu.lib.bppp_rp_open_each_device, batch, C.c_void_p(d_coms), C.c_void_p(d_amounts), C.c_void_p(d_types), C.c_void_p(d_blinds))

    def _open_each(self, fn, B, pc, pa, pt, pb):
        import ctypes as C
        import numpy as np
        nr = len(self.st.rds)
        status = np.zeros(max(B, 1) * nr, dtype=np.uint32)
        self.gpu._check(fn(self.h, B, pc, pa, pt, pb, C.c_void_p(status.ctypes.data)), "bppp_rp_open_each")
        return [[int(v) for v in status[b * nr:(b + 1) * nr]] for b in range(B)]

    def open_batch(self, coms_files: Sequence[bytes], inputs, seed: Optional[bytes] = None, want_status: bool = False, want_point: bool = False):
        """bppp_rp_open_batch: every opening checked with one weighted combination (weights: open_weight below).  `seed` is the checker's
        randomness, fresh from os.urandom unless given.  Returns accept, or (accept, statuses or None, combined point or None) when
        want_status / want_point is set: statuses as open_each returns them, the point None for the identity."""
        import ctypes as C
        B = len(inputs)
        amt, typ, bld = self._claim_arrays(inputs)
        cf = self._coms_array(coms_files, B)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        return self._open_batch(lambda *a: self.gpu.lib.bppp_rp_open_batch(self.h, B, vp(cf), vp(amt), vp(typ), vp(bld), *a), B, seed, want_status, want_point)

    def open_batch_device(self, batch: int, d_coms: int, d_amounts: int, d_types: int, d_blinds: int, seed: Optional[bytes] = None, index_offset: int = 0,
                          want_status: bool = False, want_point: bool = False):
        """bppp_rp_open_batch_device: open_batch on buffers in HBM; this call holds rows [index_offset, index_offset + batch) of a sharded job
        whose ranks all pass the same seed (their combined points add up to the one-call point)"""
        import ctypes as C
        fn = lambda *a: self.gpu.lib.bppp_rp_open_batch_device(self.h, batch, index_offset, C.c_void_p(d_coms), C.c_void_p(d_amounts), C.c_void_p(d_types),
                                                               C.c_void_p(d_blinds), *a)
        return self._open_batch(fn, batch, seed, want_status, want_point)

    def _open_batch(self, fn, B, seed, want_status, want_point):
        import ctypes as C
        import numpy as np
        from .capi import array_to_point
        if seed is None:
            seed = os.urandom(32)
        if len(seed) != 32:
            raise ValueError("a 32-byte seed is required")
        nr = len(self.st.rds)
        acc, sd = C.c_int(0), np.frombuffer(seed, dtype=np.uint8)
        status, xy = np.zeros(max(B, 1) * nr, dtype=np.uint32), np.zeros(8, dtype=np.uint64)
        rc = fn(C.c_void_p(sd.ctypes.data), C.byref(acc), C.c_void_p(status.ctypes.data) if want_status else None, C.c_void_p(xy.ctypes.data) if want_point else None)
        self.gpu._check(rc, "bppp_rp_open_batch")
        if not (want_status or want_point):
            return bool(acc.value)
        return (bool(acc.value), [[int(v) for v in status[b * nr:(b + 1) * nr]] for b in range(B)] if want_status else None,
                array_to_point(xy) if want_point else None)

    # ---- tallies: signed sums of commitments against claimed openings (bppp_rp_tally_each / bppp_rp_tally_batch / bppp_rp_tally_claims)
    @staticmethod
    def _tally_csr(sum_start, entries):
        """the CSR arrays as the entry points take them: sum_start [nsums + 1], entries [nnz] (bit 31 = subtract), both uint32"""
        import numpy as np
        if len(sum_start) < 1:
            raise ValueError("sum_start holds nsums + 1 offsets")
        return np.array(list(sum_start), dtype=np.uint32), np.array(list(entries) or [0], dtype=np.uint32), len(sum_start) - 1, len(entries)

    def _tally_claim_arrays(self, claims, nsums):
        """one (amount, type, blinding) per sum ((amount, blinding) on a binary handle) as three [nsums][4] word arrays; None: no arrays, every
        claim is zero.  Amounts are reduced mod N here (any integer names its residue); types and blindings are passed as given."""
        from .capi import scalars_to_array
        if claims is None:
            return None, None, None
        if len(claims) != nsums:
            raise ValueError("one claim per sum is required")
        rows = self._prove_rows([list(claims)])[0]
        return (scalars_to_array([tally_amount_word(a) for a, _, _ in rows] or [0]), scalars_to_array([t for _, t, _ in rows] or [0]),
                scalars_to_array([e for _, _, e in rows] or [0]))

    def tally_each(self, coms_files: Sequence[bytes], sum_start, entries, claims=None, want_points: bool = False):
        """bppp_rp_tally_each: does sum t of the commitments gathered from `coms_files` (entry = flat index row * nranges + i, bit 31 set to
        subtract: tally_entry) equal claims[t]?  Returns one capi.RP_OPEN_* per sum, or (statuses, points) with want_points: the signed sums
        themselves, None for the identity and for a MALFORMED sum.  claims None: every claim is zero."""
        import ctypes as C
        ss, en, nsums, nnz = self._tally_csr(sum_start, entries)
        amt, typ, bld = self._tally_claim_arrays(claims, nsums)
        cf = self._coms_array(coms_files, len(coms_files))
        vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        return self._tally_each(self.gpu.lib.bppp_rp_tally_each, len(coms_files), vp(cf), nsums, vp(ss), vp(en), nnz, vp(amt), vp(typ), vp(bld), want_points)

    def tally_each_device(self, rows: int, d_coms: int, nsums: int, d_sum_start: int, d_entries: int, nnz: int, d_amounts: int, d_types: int, d_blinds: int,
                          want_points: bool = False):
        """bppp_rp_tally_each_device: tally_each on buffers already in HBM (device pointers; 0 for all three claim arrays: zero claims)"""
        import ctypes as C
        p = C.c_void_p
        return self._tally_each(self.gpu.lib.bppp_rp_tally_each_device, rows, p(d_coms), nsums, p(d_sum_start), p(d_entries), nnz, p(d_amounts), p(d_types), p(d_blinds),
                                want_points)

    def _tally_each(self, fn, rows, pc, nsums, ps, pe, nnz, pa, pt, pb, want_points):
        import ctypes as C
        import numpy as np
        from .capi import array_to_point
        status, xy = np.zeros(max(nsums, 1), dtype=np.uint32), np.zeros((max(nsums, 1), 8), dtype=np.uint64)
        self.gpu._check(fn(self.h, rows, pc, nsums, ps, pe, nnz, pa, pt, pb, C.c_void_p(status.ctypes.data), C.c_void_p(xy.ctypes.data) if want_points else None),
                        "bppp_rp_tally_each")
        out = [int(v) for v in status[:nsums]]
        return (out, [array_to_point(xy[t]) for t in range(nsums)]) if want_points else out

    def tally_batch(self, coms_files: Sequence[bytes], sum_start, entries, claims=None, seed: Optional[bytes] = None, want_status: bool = False,
                    want_point: bool = False):
        """bppp_rp_tally_batch: every sum checked with one weighted combination (weights: tally_weight below).  `seed` is the checker's
        randomness, fresh from os.urandom unless given; the pool and the entries are the checker's own, fixed before the seed is drawn.
        Returns accept, or (accept, statuses or None, combined point or None) when want_status / want_point is set."""
        import ctypes as C
        ss, en, nsums, nnz = self._tally_csr(sum_start, entries)
        amt, typ, bld = self._tally_claim_arrays(claims, nsums)
        cf = self._coms_array(coms_files, len(coms_files))
        vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        fn = lambda *a: self.gpu.lib.bppp_rp_tally_batch(self.h, len(coms_files), vp(cf), nsums, vp(ss), vp(en), nnz, vp(amt), vp(typ), vp(bld), *a)
        return self._tally_batch(fn, nsums, seed, want_status, want_point)

    def tally_batch_device(self, rows: int, d_coms: int, nsums: int, d_sum_start: int, d_entries: int, nnz: int, d_amounts: int, d_types: int, d_blinds: int,
                           seed: Optional[bytes] = None, index_offset: int = 0, want_status: bool = False, want_point: bool = False):
        """bppp_rp_tally_batch_device: tally_batch on buffers in HBM; this call holds sums [index_offset, index_offset + nsums) of a sharded job
        whose ranks all pass the same seed (their combined points add up to the one-call point)"""
        import ctypes as C
        p = C.c_void_p
        fn = lambda *a: self.gpu.lib.bppp_rp_tally_batch_device(self.h, rows, p(d_coms), nsums, p(d_sum_start), p(d_entries), nnz, p(d_amounts), p(d_types), p(d_blinds),
                                                                index_offset, *a)
        return self._tally_batch(fn, nsums, seed, want_status, want_point)

    def _tally_batch(self, fn, nsums, seed, want_status, want_point):
        import ctypes as C
        import numpy as np
        from .capi import array_to_point
        if seed is None:
            seed = os.urandom(32)
        if len(seed) != 32:
            raise ValueError("a 32-byte seed is required")
        acc, sd = C.c_int(0), np.frombuffer(seed, dtype=np.uint8)
        status, xy = np.zeros(max(nsums, 1), dtype=np.uint32), np.zeros(8, dtype=np.uint64)
        rc = fn(C.c_void_p(sd.ctypes.data), C.byref(acc), C.c_void_p(status.ctypes.data) if want_status else None, C.c_void_p(xy.ctypes.data) if want_point else None)
        self.gpu._check(rc, "bppp_rp_tally_batch")
        if not (want_status or want_point):
            return bool(acc.value)
        return bool(acc.value), ([int(v) for v in status[:nsums]] if want_status else None), (array_to_point(xy) if want_point else None)

    def tally_claims(self, inputs, sum_start, entries):
        """bppp_rp_tally_claims: the claims of the signed sums over the witness rows `inputs` (commit_batch's shape): one (amount, type,
        blinding) per sum ((amount, blinding) on a binary handle), every value in [0, N).  tally_each over commit_batch(inputs) with them
        is all RP_OPEN_OK."""
        import ctypes as C
        import numpy as np
        from .capi import array_to_scalars
        ss, en, nsums, nnz = self._tally_csr(sum_start, entries)
        amt, typ, bld = self._claim_arrays(inputs)
        out = [np.zeros((max(nsums, 1), 4), dtype=np.uint64) for _ in range(3)]
        vp = lambda a: C.c_void_p(a.ctypes.data)
        rc = self.gpu.lib.bppp_rp_tally_claims(self.h, len(inputs), vp(amt), vp(typ), vp(bld), nsums, vp(ss), vp(en), nnz, vp(out[0]), vp(out[1]), vp(out[2]))
        self.gpu._check(rc, "bppp_rp_tally_claims")
        a, ty, e = (array_to_scalars(o)[:nsums] for o in out)
        return self._tally_claims_shape([((v - 2**256 if v >= 2**255 else v) % N, t, b) for v, t, b in zip(a, ty, e)])

    def _tally_claims_shape(self, triples):
        return triples

    def tally_claims_device(self, rows: int, d_amounts: int, d_types: int, d_blinds: int, nsums: int, d_sum_start: int, d_entries: int, nnz: int,
                            d_claim_amounts: int, d_claim_types: int, d_claim_blinds: int):
        """bppp_rp_tally_claims_device: tally_claims with every buffer in HBM; the three claim arrays [nsums][4] are written as the other tally
        entry points take them (d_types and d_claim_types are 0 on a binary handle)"""
        import ctypes as C
        p = C.c_void_p
        rc = self.gpu.lib.bppp_rp_tally_claims_device(self.h, rows, p(d_amounts), p(d_types), p(d_blinds), nsums, p(d_sum_start), p(d_entries), nnz, p(d_claim_amounts),
                                                      p(d_claim_types), p(d_claim_blinds))
        self.gpu._check(rc, "bppp_rp_tally_claims_device")

    # ---- excess signatures: a tally checked without revealing the blinding sum (bppp_rp_excess_sign / _verify_each / _verify_batch)
    @staticmethod
    def _excess_bytes(rows, width, what):
        import numpy as np
        if any(len(r) != width for r in rows):
            raise ValueError("%s of %d bytes each are required" % (what, width))
        return np.frombuffer(b"".join(rows) or b"\0", dtype=np.uint8)

    def _excess_claim_arrays(self, claims, nsums):
        """the public claims, one (amount, type) per sum ((amount,) or a plain amount on a binary handle; longer tuples are cut), as two
        [nsums][4] word arrays; None: no arrays, every claim is zero"""
        from .capi import scalars_to_array
        if claims is None:
            return None, None
        if len(claims) != nsums:
            raise ValueError("one claim per sum is required")
        rows = [c if isinstance(c, (tuple, list)) else (c,) for c in claims]
        typed = isinstance(self.st, SetupTRRP)
        return (scalars_to_array([tally_amount_word(c[0]) for c in rows] or [0]), scalars_to_array([c[1] for c in rows] or [0]) if typed else None)

    def excess_sign(self, blinds: Sequence[int], msgs: Sequence[bytes], aux: bytes = bytes(32), want_status: bool = False, want_points: bool = False):
        """bppp_rp_excess_sign: one signature per sum over msgs[t] with the blinding sum blinds[t] (tally_claims' last component).  Returns the
        65-byte signatures, or (signatures, statuses or None, excess points or None) as asked; without want_status a refused sum raises BpppError."""
        import ctypes as C
        import numpy as np
        from .capi import scalars_to_array
        n = len(blinds)
        if len(msgs) != n or len(aux) != 32:
            raise ValueError("one 32-byte message per sum and 32 bytes of aux are required")
        bl, mg = scalars_to_array(list(blinds) or [0]), self._excess_bytes(msgs, 32, "messages")
        sg = np.zeros(max(n, 1) * EXCESS_SIG_BYTES, dtype=np.uint8)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        return self._excess_sign(self.gpu.lib.bppp_rp_excess_sign, n, vp(bl), vp(mg), aux, vp(sg), want_status, want_points, lambda: sg)

    def excess_sign_device(self, nsums: int, d_blinds: int, d_msgs: int, d_sigs: int, aux: bytes = bytes(32), want_status: bool = False, want_points: bool = False):
        """bppp_rp_excess_sign_device: excess_sign on buffers in HBM (d_sigs receives [nsums][65] bytes); returns (statuses or None, points or None)"""
        import ctypes as C
        p = C.c_void_p
        return self._excess_sign(self.gpu.lib.bppp_rp_excess_sign_device, nsums, p(d_blinds), p(d_msgs), aux, p(d_sigs), want_status, want_points, None)

    def _excess_sign(self, fn, n, pb, pm, aux, ps, want_status, want_points, sigs):
        import ctypes as C
        import numpy as np
        from .capi import array_to_point
        status, xy, ax = np.zeros(max(n, 1), dtype=np.uint32), np.zeros((max(n, 1), 8), dtype=np.uint64), np.frombuffer(aux, dtype=np.uint8)
        rc = fn(self.h, n, pb, pm, C.c_void_p(ax.ctypes.data), ps, C.c_void_p(xy.ctypes.data) if want_points else None, C.c_void_p(status.ctypes.data) if want_status else None)
        self.gpu._check(rc, "bppp_rp_excess_sign")
        st = [int(v) for v in status[:n]] if want_status else None
        pts = [array_to_point(xy[t]) for t in range(n)] if want_points else None
        if sigs is None:
            return st, pts
        raw = sigs().tobytes()
        out = [raw[t * EXCESS_SIG_BYTES:(t + 1) * EXCESS_SIG_BYTES] for t in range(n)]
        return (out, st, pts) if (want_status or want_points) else out

    def _excess_host_args(self, coms_files, sum_start, entries, claims, msgs, sigs):
        import ctypes as C
        ss, en, nsums, nnz = self._tally_csr(sum_start, entries)
        if len(msgs) != nsums or len(sigs) != nsums:
            raise ValueError("one message and one signature per sum are required")
        amt, typ = self._excess_claim_arrays(claims, nsums)
        keep = [self._coms_array(coms_files, len(coms_files)), ss, en, amt, typ, self._excess_bytes(msgs, 32, "messages"), self._excess_bytes(sigs, EXCESS_SIG_BYTES, "signatures")]
        vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        cf, ss, en, amt, typ, mg, sg = keep
        return keep, nsums, (len(coms_files), vp(cf), nsums, vp(ss), vp(en), nnz, vp(amt), vp(typ), vp(mg), vp(sg))

    def excess_verify_each(self, coms_files: Sequence[bytes], sum_start, entries, claims, msgs: Sequence[bytes], sigs: Sequence[bytes], want_points: bool = False):
        """bppp_rp_excess_verify_each: does sigs[t] sign msgs[t] under the excess of sum t over the public claims[t] ((amount, type); a binary
        handle: the amount)?  Returns one verdict per sum (capi.RP_OPEN_* / RP_EXCESS_BAD_R / RP_EXCESS_NO_KEY), or (verdicts, excess points)."""
        keep, nsums, args = self._excess_host_args(coms_files, sum_start, entries, claims, msgs, sigs)
        return self._excess_each(self.gpu.lib.bppp_rp_excess_verify_each, nsums, args, want_points)

    def excess_verify_each_device(self, rows: int, d_coms: int, nsums: int, d_sum_start: int, d_entries: int, nnz: int, d_amounts: int, d_types: int, d_msgs: int,
                                  d_sigs: int, want_points: bool = False):
        """bppp_rp_excess_verify_each_device: excess_verify_each on buffers in HBM (0 for both claim arrays: zero claims)"""
        import ctypes as C
        p = C.c_void_p
        return self._excess_each(self.gpu.lib.bppp_rp_excess_verify_each_device, nsums,
                                 (rows, p(d_coms), nsums, p(d_sum_start), p(d_entries), nnz, p(d_amounts), p(d_types), p(d_msgs), p(d_sigs)), want_points)

    def _excess_each(self, fn, nsums, args, want_points):
        import ctypes as C
        import numpy as np
        from .capi import array_to_point
        status, xy = np.zeros(max(nsums, 1), dtype=np.uint32), np.zeros((max(nsums, 1), 8), dtype=np.uint64)
        self.gpu._check(fn(self.h, *args, C.c_void_p(status.ctypes.data), C.c_void_p(xy.ctypes.data) if want_points else None), "bppp_rp_excess_verify_each")
        out = [int(v) for v in status[:nsums]]
        return (out, [array_to_point(xy[t]) for t in range(nsums)]) if want_points else out

    def excess_verify_batch(self, coms_files: Sequence[bytes], sum_start, entries, claims, msgs: Sequence[bytes], sigs: Sequence[bytes], seed: Optional[bytes] = None,
                            want_status: bool = False, want_point: bool = False):
        """bppp_rp_excess_verify_batch: every signature checked with one weighted combination (weights: excess_weight below).  Returns accept, or
        (accept, verdicts or None, combined point or None) when want_status / want_point is set."""
        keep, nsums, args = self._excess_host_args(coms_files, sum_start, entries, claims, msgs, sigs)
        fn = lambda *a: self.gpu.lib.bppp_rp_excess_verify_batch(self.h, *args, *a)
        return self._tally_batch(fn, nsums, seed, want_status, want_point)

    def excess_verify_batch_device(self, rows: int, d_coms: int, nsums: int, d_sum_start: int, d_entries: int, nnz: int, d_amounts: int, d_types: int, d_msgs: int,
                                   d_sigs: int, seed: Optional[bytes] = None, index_offset: int = 0, want_status: bool = False, want_point: bool = False):
        """bppp_rp_excess_verify_batch_device: excess_verify_batch on buffers in HBM; this call holds sums [index_offset, index_offset + nsums) of a
        sharded job whose ranks all pass the same seed (their combined points add up to the one-call point)"""
        import ctypes as C
        p = C.c_void_p
        fn = lambda *a: self.gpu.lib.bppp_rp_excess_verify_batch_device(self.h, rows, p(d_coms), nsums, p(d_sum_start), p(d_entries), nnz, p(d_amounts), p(d_types),
                                                                        p(d_msgs), p(d_sigs), index_offset, *a)
        return self._tally_batch(fn, nsums, seed, want_status, want_point)

    # ---- excess keys: the excess stated as 33 bytes, for signatures checked with no pool and sums checked after cut-through
    # (bppp_rp_excess_keys / _verify_keys_each / _verify_keys_batch / _sums_each / _sums_batch)
    def excess_keys(self, blinds: Sequence[int], want_status: bool = False):
        """bppp_rp_excess_keys: the 33-byte key X = e B of every blinding sum.  Returns the keys, or (keys, statuses) with want_status (a refused
        sum has 33 zero bytes); without it a refused sum raises BpppError."""
        import ctypes as C
        import numpy as np
        from .capi import scalars_to_array
        n = len(blinds)
        bl, ks = scalars_to_array(list(blinds) or [0]), np.zeros(max(n, 1) * EXCESS_KEY_BYTES, dtype=np.uint8)
        st = self._excess_keys(self.gpu.lib.bppp_rp_excess_keys, n, C.c_void_p(bl.ctypes.data), C.c_void_p(ks.ctypes.data), want_status)
        raw = ks.tobytes()
        out = [raw[t * EXCESS_KEY_BYTES:(t + 1) * EXCESS_KEY_BYTES] for t in range(n)]
        return (out, st) if want_status else out

    def excess_keys_device(self, nsums: int, d_blinds: int, d_keys: int, want_status: bool = False):
        """bppp_rp_excess_keys_device: excess_keys on buffers in HBM (d_keys receives [nsums][33] bytes); returns the statuses or None"""
        import ctypes as C
        return self._excess_keys(self.gpu.lib.bppp_rp_excess_keys_device, nsums, C.c_void_p(d_blinds), C.c_void_p(d_keys), want_status)

    def _excess_keys(self, fn, n, pb, pk, want_status):
        import ctypes as C
        import numpy as np
        status = np.zeros(max(n, 1), dtype=np.uint32)
        self.gpu._check(fn(self.h, n, pb, pk, C.c_void_p(status.ctypes.data) if want_status else None), "bppp_rp_excess_keys")
        return [int(v) for v in status[:n]] if want_status else None

    # ---- sealed outputs: a one-sided receive and the view-key scan (bppp_rp_seal / bppp_rp_scan)
    def seal(self, view_keys: Sequence[bytes], eph: Sequence[int], outputs, want_status: bool = False):
        """bppp_rp_seal: row b is sealed to the 33-byte view key view_keys[b] under the ephemeral secret eph[b]; outputs[b] = one (amount, type) per
        range (the type is ignored on a binary handle).  Returns (seals, blinds) — the seal's bytes and the blindings to commit or prove with, one
        list per row — or (seals, blinds, statuses) with want_status (a refused row has zero bytes and zero blindings); without it a refused row
        raises BpppError."""
        import ctypes as C
        import numpy as np
        from .capi import array_to_scalars, scalars_to_array
        B, nr, sb = len(outputs), len(self.st.rds), SEAL_BYTES(len(self.st.rds))
        if len(view_keys) != B or len(eph) != B or any(len(k) != EXCESS_KEY_BYTES for k in view_keys) or any(len(row) != nr for row in outputs):
            raise ValueError("one 33-byte view key, one ephemeral secret and one (amount, type) per range are required per row")
        if B == 0:
            return ([], [], []) if want_status else ([], [])
        keys = np.frombuffer(b"".join(view_keys), dtype=np.uint8)
        e, amt = scalars_to_array(list(eph)), scalars_to_array([v % 2**256 for row in outputs for v, _ in row])
        typ = scalars_to_array([t for row in outputs for _, t in row])
        seals, blinds, status = np.zeros(B * sb, dtype=np.uint8), np.zeros((B * nr, 4), dtype=np.uint64), np.zeros(B, dtype=np.uint32)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        rc = self.gpu.lib.bppp_rp_seal(self.h, B, vp(keys), vp(e), vp(amt), vp(typ), vp(seals), vp(blinds), vp(status) if want_status else None)
        self.gpu._check(rc, "bppp_rp_seal")
        bl = array_to_scalars(blinds)
        out = ([seals[b * sb:(b + 1) * sb].tobytes() for b in range(B)], [bl[b * nr:(b + 1) * nr] for b in range(B)])
        return out + ([int(s) for s in status],) if want_status else out

    def seal_device(self, batch: int, d_view_keys: int, d_eph: int, d_amounts: int, d_types: int, d_seals: int, d_blinds: int, want_status: bool = False):
        """bppp_rp_seal_device: seal on buffers in HBM (device pointers; d_types is 0 on a binary handle); d_seals receives [batch][SEAL_BYTES] bytes and
        d_blinds [batch][nranges][4] words.  Returns the verdicts (numpy uint32 [batch]) with want_status, else None (a refused row raises)."""
        import ctypes as C
        import numpy as np
        status = np.zeros(max(batch, 1), dtype=np.uint32)
        rc = self.gpu.lib.bppp_rp_seal_device(self.h, batch, C.c_void_p(d_view_keys), C.c_void_p(d_eph), C.c_void_p(d_amounts), C.c_void_p(d_types), C.c_void_p(d_seals),
                                              C.c_void_p(d_blinds), C.c_void_p(status.ctypes.data) if want_status else None)
        self.gpu._check(rc, "bppp_rp_seal_device")
        return status[:batch] if want_status else None

    def scan(self, view_secret: int, coms_files: Sequence[bytes], seals: Sequence[bytes]):
        """bppp_rp_scan: the rows of (commitments file, seal) that belong to the view secret.  Returns (statuses, openings, nowned): capi.RP_SCAN_* per
        row, and per row one (amount, type, blinding) per range — the amount as the scalar in [0, n) — all zeros unless the row is owned."""
        import ctypes as C
        import numpy as np
        from .capi import array_to_scalars, int_to_limbs
        rows, nr, sb = len(seals), len(self.st.rds), SEAL_BYTES(len(self.st.rds))
        if any(len(s) != sb for s in seals):
            raise ValueError("every seal has SEAL_BYTES (nranges) bytes")
        a = int_to_limbs(view_secret % 2**256)
        cf = self._coms_array(coms_files, rows)
        sl = np.frombuffer(b"".join(seals) or b"\0", dtype=np.uint8)
        status = np.zeros(max(rows, 1), dtype=np.uint32)
        out = [np.zeros((max(rows, 1) * nr, 4), dtype=np.uint64) for _ in range(3)]
        nowned = C.c_size_t(0)
        vp = lambda x: C.c_void_p(x.ctypes.data)
        rc = self.gpu.lib.bppp_rp_scan(self.h, vp(a), rows, vp(cf), vp(sl), vp(status), vp(out[0]), vp(out[1]), vp(out[2]), C.byref(nowned))
        self.gpu._check(rc, "bppp_rp_scan")
        v, t, bl = (array_to_scalars(o) for o in out)
        return ([int(s) for s in status[:rows]], [[(v[b * nr + i], t[b * nr + i], bl[b * nr + i]) for i in range(nr)] for b in range(rows)], int(nowned.value))

    def scan_device(self, view_secret: int, rows: int, d_coms: int, d_seals: int, d_amounts: int = 0, d_types: int = 0, d_blinds: int = 0):
        """bppp_rp_scan_device: scan on buffers in HBM (device pointers; an output pointer of 0 is not written).  Returns (statuses as numpy uint32
        [rows], nowned)."""
        import ctypes as C
        import numpy as np
        from .capi import int_to_limbs
        a = int_to_limbs(view_secret % 2**256)
        status, nowned = np.zeros(max(rows, 1), dtype=np.uint32), C.c_size_t(0)
        rc = self.gpu.lib.bppp_rp_scan_device(self.h, C.c_void_p(a.ctypes.data), rows, C.c_void_p(d_coms), C.c_void_p(d_seals), C.c_void_p(status.ctypes.data),
                                              C.c_void_p(d_amounts), C.c_void_p(d_types), C.c_void_p(d_blinds), C.byref(nowned))
        self.gpu._check(rc, "bppp_rp_scan_device")
        return status[:rows], int(nowned.value)

    # ---- the scan under many view secrets (bppp_rp_scan_keys)
    def _scan_keys_hits(self, nhits: int, cap: int, hit_key, hit_row, v, t, bl):
        nr, n = len(self.st.rds), min(nhits, cap)
        return [(int(hit_key[h]), int(hit_row[h]), [(v[h * nr + i], t[h * nr + i], bl[h * nr + i]) for i in range(nr)]) for h in range(n)]

    def scan_keys(self, view_secrets: Sequence[int], coms_files: Sequence[bytes], seals: Sequence[bytes]):
        """bppp_rp_scan_keys: the rows of (commitments file, seal) under every secret of view_secrets in one call.  Returns (row_status, hits,
        ntag_only): capi.RP_SCAN_* per row (BAD_HINT, else OWNED if some key owns it, else TAG_ONLY if some key's tag matched, else FOREIGN), the
        hits as (key, row, opening) ordered by (row, key) with opening = one (amount, type, blinding) per range, and the number of (key, row) pairs
        whose tag matched without the row opening.  Starts with cap = rows and calls once more with cap = nhits if that was too small."""
        import ctypes as C
        import numpy as np
        from .capi import array_to_scalars, scalars_to_array
        rows, nr, sb = len(seals), len(self.st.rds), SEAL_BYTES(len(self.st.rds))
        if any(len(s) != sb for s in seals):
            raise ValueError("every seal has SEAL_BYTES (nranges) bytes")
        keys = scalars_to_array([a % 2**256 for a in view_secrets]) if len(view_secrets) else np.zeros((1, 4), dtype=np.uint64)
        cf = self._coms_array(coms_files, rows)
        sl = np.frombuffer(b"".join(seals) or b"\0", dtype=np.uint8)
        status = np.zeros(max(rows, 1), dtype=np.uint32)
        vp = lambda x: C.c_void_p(x.ctypes.data)
        cap = rows
        while True:
            hk, hr = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint32)
            out = [np.zeros((max(cap, 1) * nr, 4), dtype=np.uint64) for _ in range(3)]
            nhits, ntag = C.c_size_t(0), C.c_uint64(0)
            rc = self.gpu.lib.bppp_rp_scan_keys(self.h, len(view_secrets), vp(keys), rows, vp(cf), vp(sl), vp(status), cap, vp(hk), vp(hr), vp(out[0]), vp(out[1]), vp(out[2]),
                                                C.byref(nhits), C.byref(ntag))
            self.gpu._check(rc, "bppp_rp_scan_keys")
            if nhits.value <= cap:
                break
            cap = nhits.value
        hits = self._scan_keys_hits(nhits.value, cap, hk, hr, *(array_to_scalars(o) for o in out))
        return [int(s) for s in status[:rows]], hits, int(ntag.value)

    def scan_keys_device(self, view_secrets: Sequence[int], rows: int, d_coms: int, d_seals: int):
        """bppp_rp_scan_keys_device: the same on files and seals in HBM (device pointers).  The hit list's openings are written to HBM buffers of this
        call's own and downloaded, so the result is scan_keys': (row_status, hits, ntag_only).  Starts with cap = rows, once more with cap = nhits."""
        import ctypes as C
        import numpy as np
        from .capi import array_to_scalars, scalars_to_array
        nr, g = len(self.st.rds), self.gpu
        keys = scalars_to_array([a % 2**256 for a in view_secrets]) if len(view_secrets) else np.zeros((1, 4), dtype=np.uint64)
        status = np.zeros(max(rows, 1), dtype=np.uint32)
        vp = lambda x: C.c_void_p(x.ctypes.data)
        cap = rows
        while True:
            hk, hr = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint32)
            nhits, ntag = C.c_size_t(0), C.c_uint64(0)
            d_out = [g.alloc(max(cap, 1) * nr * 32) for _ in range(3)]
            try:
                rc = g.lib.bppp_rp_scan_keys_device(self.h, len(view_secrets), vp(keys), rows, C.c_void_p(d_coms), C.c_void_p(d_seals), vp(status), cap, vp(hk), vp(hr),
                                                    C.c_void_p(d_out[0]), C.c_void_p(d_out[1]), C.c_void_p(d_out[2]), C.byref(nhits), C.byref(ntag))
                g._check(rc, "bppp_rp_scan_keys_device")
                out = [array_to_scalars(g.download(d, (max(cap, 1) * nr, 4), np.uint64)) for d in d_out] if nhits.value <= cap else None
            finally:
                for d in d_out:
                    g.free(d)
            if out is not None:
                break
            cap = nhits.value
        return [int(s) for s in status[:rows]], self._scan_keys_hits(nhits.value, cap, hk, hr, *out), int(ntag.value)

    def commitment_set(self, row_bytes: int, keep_nodes: bool = True) -> "CommitmentSet":
        """bppp_rp_set_create: an empty set commitment over rows of row_bytes bytes on this handle (CommitmentSet below)"""
        return CommitmentSet(self, row_bytes, keep_nodes)

    @staticmethod
    def set_path_bytes(n: int) -> int:
        """bppp_rp_set_path_bytes, asked of the library"""
        from .capi import load_library
        return int(load_library().bppp_rp_set_path_bytes(int(n)))

    def set_verify_paths(self, row_bytes: int, n: int, root: bytes, idx: Sequence[int], rows: Sequence[bytes], paths: Sequence[bytes], want_status: bool = False):
        """bppp_rp_set_verify_paths: is rows[q] leaf idx[q] of the set of n rows with this root, by paths[q]?  Stateless.  Returns accept, or
        (accept, [SET_OK / SET_MISMATCH / SET_BAD_INDEX / SET_BAD_PADDING per query]) with want_status"""
        import ctypes as C
        import numpy as np
        nq, pb = len(idx), set_path_bytes(n)
        if len(rows) != nq or len(paths) != nq or any(len(r) != row_bytes for r in rows) or any(len(p) != pb for p in paths) or len(root) != 32:
            raise ValueError("one row of row_bytes bytes and one path of 32 bit_length (n) bytes per index, and a root of 32 bytes")
        ix = np.array([int(i) % 2**64 for i in idx] or [0], dtype=np.uint64)
        rw = np.frombuffer(b"".join(rows) or b"\0", dtype=np.uint8)
        pt = np.frombuffer(b"".join(paths) or b"\0", dtype=np.uint8)
        rt = np.frombuffer(bytes(root), dtype=np.uint8)
        st = np.zeros(max(nq, 1), dtype=np.uint32)
        accept = C.c_int(-1)
        vp = lambda x: C.c_void_p(x.ctypes.data)
        rc = self.gpu.lib.bppp_rp_set_verify_paths(self.h, row_bytes, n, vp(rt), nq, vp(ix), vp(rw), vp(pt) if pb else None, vp(st) if want_status else None, C.byref(accept))
        self.gpu._check(rc, "bppp_rp_set_verify_paths")
        return (bool(accept.value), [int(v) for v in st[:nq]]) if want_status else bool(accept.value)

    def _excess_key_args(self, keys, msgs, sigs):
        import ctypes as C
        n = len(keys)
        if len(msgs) != n or len(sigs) != n:
            raise ValueError("one message and one signature per key are required")
        keep = [self._excess_bytes(keys, EXCESS_KEY_BYTES, "keys"), self._excess_bytes(msgs, 32, "messages"), self._excess_bytes(sigs, EXCESS_SIG_BYTES, "signatures")]
        return keep, n, (n,) + tuple(C.c_void_p(a.ctypes.data) for a in keep)

    def excess_verify_keys_each(self, keys: Sequence[bytes], msgs: Sequence[bytes], sigs: Sequence[bytes]):
        """bppp_rp_excess_verify_keys_each: does sigs[t] sign msgs[t] under the stated key keys[t]?  No pool is needed.  Returns one verdict per key
        (capi.RP_OPEN_OK / _MISMATCH / _NOT_CANONICAL, RP_EXCESS_BAD_R, RP_EXCESS_BAD_KEY)."""
        keep, n, args = self._excess_key_args(keys, msgs, sigs)
        return self._excess_keys_each(self.gpu.lib.bppp_rp_excess_verify_keys_each, n, args)

    def excess_verify_keys_each_device(self, nkeys: int, d_keys: int, d_msgs: int, d_sigs: int):
        """bppp_rp_excess_verify_keys_each_device: excess_verify_keys_each on buffers in HBM"""
        import ctypes as C
        p = C.c_void_p
        return self._excess_keys_each(self.gpu.lib.bppp_rp_excess_verify_keys_each_device, nkeys, (nkeys, p(d_keys), p(d_msgs), p(d_sigs)))

    def _excess_keys_each(self, fn, n, args):
        import ctypes as C
        import numpy as np
        status = np.zeros(max(n, 1), dtype=np.uint32)
        self.gpu._check(fn(self.h, *args, C.c_void_p(status.ctypes.data)), "bppp_rp_excess_verify_keys_each")
        return [int(v) for v in status[:n]]

    def excess_verify_keys_batch(self, keys: Sequence[bytes], msgs: Sequence[bytes], sigs: Sequence[bytes], seed: Optional[bytes] = None, want_status: bool = False,
                                 want_point: bool = False):
        """bppp_rp_excess_verify_keys_batch: every signature under its stated key with one weighted combination (weights: excess_weight over the lifted
        key).  Returns accept, or (accept, verdicts or None, combined point or None) when want_status / want_point is set."""
        keep, n, args = self._excess_key_args(keys, msgs, sigs)
        fn = lambda *a: self.gpu.lib.bppp_rp_excess_verify_keys_batch(self.h, *args, *a)
        return self._tally_batch(fn, n, seed, want_status, want_point)

    def excess_verify_keys_batch_device(self, nkeys: int, d_keys: int, d_msgs: int, d_sigs: int, seed: Optional[bytes] = None, index_offset: int = 0,
                                        want_status: bool = False, want_point: bool = False):
        """bppp_rp_excess_verify_keys_batch_device: excess_verify_keys_batch on buffers in HBM; this call holds keys [index_offset, index_offset + nkeys) of a
        sharded job whose ranks all pass the same seed (their combined points add up to the one-call point)"""
        import ctypes as C
        p = C.c_void_p
        fn = lambda *a: self.gpu.lib.bppp_rp_excess_verify_keys_batch_device(self.h, nkeys, p(d_keys), p(d_msgs), p(d_sigs), index_offset, *a)
        return self._tally_batch(fn, nkeys, seed, want_status, want_point)

    def _excess_sums_host_args(self, coms_files, sum_start, entries, claims, key_start, keys):
        import ctypes as C
        import numpy as np
        ss, en, nsums, nnz = self._tally_csr(sum_start, entries)
        if len(key_start) != nsums + 1:
            raise ValueError("key_start holds nsums + 1 offsets")
        amt, typ, off = self._tally_claim_arrays(claims, nsums)
        keep = [self._coms_array(coms_files, len(coms_files)), ss, en, amt, typ, off, np.array(list(key_start), dtype=np.uint32), self._excess_bytes(keys, EXCESS_KEY_BYTES, "keys")]
        vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        cf, ss, en, amt, typ, off, ks, ky = keep
        return keep, nsums, (len(coms_files), vp(cf), nsums, vp(ss), vp(en), nnz, vp(amt), vp(typ), vp(off), len(keys), vp(ks), vp(ky))

    def excess_sums_each(self, coms_files: Sequence[bytes], sum_start, entries, claims, key_start, keys: Sequence[bytes], want_points: bool = False):
        """bppp_rp_excess_sums_each: does sum t, less claims[t] = (amount, type, offset) ((amount, offset) on a binary handle; None: zero claims), equal
        the sum of the stated keys keys[key_start[t]:key_start[t + 1]]?  Returns one verdict per sum (capi.RP_OPEN_* / RP_EXCESS_BAD_KEY), or (verdicts,
        points) with want_points: S_t less its keys, None for the identity, a MALFORMED and a BAD_KEY sum."""
        keep, nsums, args = self._excess_sums_host_args(coms_files, sum_start, entries, claims, key_start, keys)
        return self._excess_each(self.gpu.lib.bppp_rp_excess_sums_each, nsums, args, want_points)

    def excess_sums_each_device(self, rows: int, d_coms: int, nsums: int, d_sum_start: int, d_entries: int, nnz: int, d_amounts: int, d_types: int, d_offsets: int,
                                nkeys: int, d_key_start: int, d_keys: int, want_points: bool = False):
        """bppp_rp_excess_sums_each_device: excess_sums_each on buffers in HBM (0 for all three claim arrays: zero claims)"""
        import ctypes as C
        p = C.c_void_p
        return self._excess_each(self.gpu.lib.bppp_rp_excess_sums_each_device, nsums,
                                 (rows, p(d_coms), nsums, p(d_sum_start), p(d_entries), nnz, p(d_amounts), p(d_types), p(d_offsets), nkeys, p(d_key_start), p(d_keys)), want_points)

    def excess_sums_batch(self, coms_files: Sequence[bytes], sum_start, entries, claims, key_start, keys: Sequence[bytes], seed: Optional[bytes] = None,
                          want_status: bool = False, want_point: bool = False):
        """bppp_rp_excess_sums_batch: every sum against its stated keys with one weighted combination (weights: tally_weight over (amount, type,
        offset)).  Returns accept, or (accept, verdicts or None, combined point or None) when want_status / want_point is set."""
        keep, nsums, args = self._excess_sums_host_args(coms_files, sum_start, entries, claims, key_start, keys)
        fn = lambda *a: self.gpu.lib.bppp_rp_excess_sums_batch(self.h, *args, *a)
        return self._tally_batch(fn, nsums, seed, want_status, want_point)

    def excess_sums_batch_device(self, rows: int, d_coms: int, nsums: int, d_sum_start: int, d_entries: int, nnz: int, d_amounts: int, d_types: int, d_offsets: int,
                                 nkeys: int, d_key_start: int, d_keys: int, seed: Optional[bytes] = None, index_offset: int = 0, want_status: bool = False,
                                 want_point: bool = False):
        """bppp_rp_excess_sums_batch_device: excess_sums_batch on buffers in HBM; this call holds sums [index_offset, index_offset + nsums) of a sharded job
        whose ranks all pass the same seed (their combined points add up to the one-call point)"""
        import ctypes as C
        p = C.c_void_p
        fn = lambda *a: self.gpu.lib.bppp_rp_excess_sums_batch_device(self.h, rows, p(d_coms), nsums, p(d_sum_start), p(d_entries), nnz, p(d_amounts), p(d_types), p(d_offsets),
                                                                      nkeys, p(d_key_start), p(d_keys), index_offset, *a)
        return self._tally_batch(fn, nsums, seed, want_status, want_point)

    # ---- cut-through: the transactions' job -> the block's pool, one sum and claim (bppp_rp_cut_through / _device)
    def _cut_claims(self, words):
        """block_claims [3][4] -> the claim as verify_block takes it: (amount, type, offset) mod N ((amount, offset) on a binary handle)"""
        from .capi import array_to_scalars
        a, ty, o = array_to_scalars(words)
        return self._tally_claims_shape([((a - 2**256 if a >= 2**255 else a) % N, ty, o)])[0]

    def _cut_call(self, fn, name, rows, pc, nsums, ps, pe, nnz, pa, pt, po, p_new_coms, p_new_entries, have_claims):
        import ctypes as C
        import numpy as np
        from .capi import RpCutCounts
        status, row_map = np.zeros(max(nnz, 1), dtype=np.uint32), np.zeros(max(rows, 1), dtype=np.uint32)
        bc, cnt = np.zeros((3, 4), dtype=np.uint64), RpCutCounts()
        vp = lambda a: C.c_void_p(a.ctypes.data)
        self.gpu._check(fn(self.h, rows, pc, nsums, ps, pe, nnz, pa, pt, po, vp(status), vp(row_map), p_new_coms, p_new_entries, vp(bc) if have_claims else None,
                           C.byref(cnt)), name)
        counts = {n: int(getattr(cnt, n)) for n, _ in RpCutCounts._fields_}
        empty = nsums == 0 or nnz == 0
        return CutThrough(None, None, [int(v) for v in row_map[:counts["new_rows"]]], counts["out_rows"], [] if empty else [int(v) for v in status[:nnz]],
                          self._cut_claims(bc) if have_claims else None, counts)

    def cut_through(self, coms_files: Sequence[bytes], sum_start, entries, claims=None) -> "CutThrough":
        """bppp_rp_cut_through: the job of T transactions (the pool, one sum per transaction, claims (amount, type, offset) per sum or None) merged
        into a block — outputs created and spent inside the set are dropped with their spends.  Returns a CutThrough: the new pool, the one sum's
        entries, row_map, out_rows, one capi.RP_CUT_* per entry, the summed claim and the counts (cut_through_host restates every rule)."""
        import ctypes as C
        import numpy as np
        ss, en, nsums, nnz = self._tally_csr(sum_start, entries)
        amt, typ, off = self._tally_claim_arrays(claims, nsums)
        rows, cb = len(coms_files), self.shape["coms_bytes"]
        cf = self._coms_array(coms_files, rows)
        nc, ne = np.zeros(max(rows * cb, 1), dtype=np.uint8), np.zeros(max(nnz, 1), dtype=np.uint32)
        vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        r = self._cut_call(self.gpu.lib.bppp_rp_cut_through, "bppp_rp_cut_through", rows, vp(cf), nsums, vp(ss), vp(en), nnz, vp(amt), vp(typ), vp(off), vp(nc), vp(ne),
                           claims is not None)
        r.coms_files = [nc[k * cb:(k + 1) * cb].tobytes() for k in range(r.counts["new_rows"])]
        r.entries = [int(v) for v in ne[:r.counts["new_nnz"]]]
        return r

    def cut_through_device(self, rows: int, d_coms: int, nsums: int, d_sum_start: int, d_entries: int, nnz: int, d_amounts: int, d_types: int, d_offsets: int,
                           d_new_coms: int, d_new_entries: int) -> "CutThrough":
        """bppp_rp_cut_through_device: cut_through on buffers in HBM (0 for all three claim arrays: no claims; d_new_coms may be 0).  The new pool and
        the one sum's entries are written to d_new_coms [rows][coms_bytes] and d_new_entries [nnz]: the CutThrough returned has None for both and
        counts["new_rows"] / counts["new_nnz"] say how much of them is filled."""
        import ctypes as C
        p = C.c_void_p
        return self._cut_call(self.gpu.lib.bppp_rp_cut_through_device, "bppp_rp_cut_through_device", rows, p(d_coms), nsums, p(d_sum_start), p(d_entries), nnz,
                              p(d_amounts), p(d_types), p(d_offsets), p(d_new_coms), p(d_new_entries), bool(d_amounts or d_offsets))

    def assemble_block(self, coms_files: Sequence[bytes], sum_start, entries, claims, keys: Sequence[bytes], msgs: Sequence[bytes], sigs: Sequence[bytes],
                       proof_files: Optional[Sequence[bytes]] = None, bindings=None):
        """The transactions' job -> the arguments of verify_block, through one cut_through: thin host glue.  proof_files (and bindings): None, or one
        per ROW of the old pool (None for a row without a proof, e.g. the copy of a spent output); what belongs to a row is gathered with row_map, and
        every new output (the rows in front of the new pool) must carry a proof.  The keys, messages and signatures of all transactions stand in one
        group.  Returns (kwargs, cut): verify_block(**kwargs) checks the block; cut is the CutThrough."""
        cut = self.cut_through(coms_files, sum_start, entries, claims)
        outs = cut.row_map[:cut.out_rows]
        proofs = [] if proof_files is None else [proof_files[r] for r in outs]
        if any(p is None for p in proofs):
            raise ValueError("every surviving output needs its proof file")
        binds = None if bindings is None or proof_files is None else [bindings[r] for r in outs]
        kwargs = dict(coms_files=cut.coms_files, proof_files=proofs, sum_start=[0, len(cut.entries)], entries=cut.entries,
                      claims=None if cut.claims is None else [cut.claims], key_start=[0, len(keys)], keys=list(keys), msgs=list(msgs), sigs=list(sigs), bindings=binds)
        return kwargs, cut

    # ---- a block in one call: range proofs, key signatures and sums after cut-through as ONE MSM (bppp_rp_verify_block / _device)
    def block_arrays(self, coms_files, proof_files, sum_start, entries, claims, key_start, keys, msgs, sigs, bindings):
        """the block's arguments as [(field of capi.RpBlock, numpy array or None)] and its sizes as a dict of RpBlock's counts: what verify_block passes
        from the host, and what a caller uploads once to fill an RpBlock with device pointers for verify_block_call(..., device=True)"""
        import numpy as np
        from .capi import bindings_array
        rows, nproofs, nkeys = len(coms_files), len(proof_files), len(keys)
        if any(len(p) != self.shape["proof_bytes"] for p in proof_files):
            raise ValueError("proof files of proof_bytes each are required")
        if len(msgs) != nkeys or len(sigs) != nkeys:
            raise ValueError("one message and one signature per key are required")
        ss, en, nsums, nnz = self._tally_csr(sum_start if sum_start is not None else [0], entries)
        if len(key_start) != nsums + 1:
            raise ValueError("key_start holds nsums + 1 offsets")
        amt, typ, off = self._tally_claim_arrays(claims, nsums)
        arrs = [("coms_files", self._coms_array(coms_files, rows)), ("proof_files", np.frombuffer(b"".join(proof_files) or b"\0", dtype=np.uint8)),
                ("bindings", None if bindings is None else bindings_array(bindings, nproofs)), ("sum_start", ss), ("entries", en), ("claim_amounts", amt),
                ("claim_types", typ), ("claim_offsets", off), ("key_start", np.array(list(key_start), dtype=np.uint32)),
                ("keys", self._excess_bytes(keys, EXCESS_KEY_BYTES, "keys")), ("msgs", self._excess_bytes(msgs, 32, "messages")),
                ("sigs", self._excess_bytes(sigs, EXCESS_SIG_BYTES, "signatures"))]
        return arrs, dict(rows=rows, nproofs=nproofs, nsums=nsums, nnz=nnz, nkeys=nkeys)

    def verify_block_call(self, blk, seed: Optional[bytes] = None, want_status: bool = False, want_point: bool = False, device: bool = False, agg: Optional[int] = None):
        """bppp_rp_verify_block (device: bppp_rp_verify_block_device) on a filled capi.RpBlock.  Returns accept, or (accept, (proof, key, sum
        statuses) or None, combined point or None) when want_status / want_point is set.  agg: the address of a half-aggregate (host memory, or HBM
        with device) — then the call is bppp_rp_verify_block_agg / _device, and blk.sigs and blk.key_offset stay zero."""
        import ctypes as C
        import numpy as np
        from .capi import RpBlockStatus, array_to_point
        if seed is None:
            seed = os.urandom(32)
        if len(seed) != 32:
            raise ValueError("a 32-byte seed is required")
        acc, sd, xy = C.c_int(0), np.frombuffer(seed, dtype=np.uint8), np.zeros(8, dtype=np.uint64)
        sts = [np.zeros(max(n, 1), dtype=np.uint32) for n in (blk.nproofs, blk.nkeys, blk.nsums)]
        status = RpBlockStatus(*[a.ctypes.data for a in sts])
        lib = self.gpu.lib
        if agg is None:
            fn, head = (lib.bppp_rp_verify_block_device if device else lib.bppp_rp_verify_block), (self.h, C.byref(blk))
        else:
            fn, head = (lib.bppp_rp_verify_block_agg_device if device else lib.bppp_rp_verify_block_agg), (self.h, C.byref(blk), C.c_void_p(agg))
        rc = fn(*head, C.c_void_p(sd.ctypes.data), C.byref(acc), C.byref(status) if want_status else None, C.c_void_p(xy.ctypes.data) if want_point else None)
        self.gpu._check(rc, "bppp_rp_verify_block")
        if not (want_status or want_point):
            return bool(acc.value)
        st = tuple([int(v) for v in a[:n]] for a, n in zip(sts, (blk.nproofs, blk.nkeys, blk.nsums))) if want_status else None
        return bool(acc.value), st, (array_to_point(xy) if want_point else None)

    def verify_block(self, coms_files: Sequence[bytes], proof_files: Sequence[bytes], sum_start, entries, claims, key_start, keys: Sequence[bytes], msgs: Sequence[bytes],
                     sigs: Sequence[bytes], bindings=None, seed: Optional[bytes] = None, offsets=(0, 0, 0), want_status: bool = False, want_point: bool = False,
                     _device: bool = False):
        """bppp_rp_verify_block: a block in one call and one MSM.  coms_files: the pool, its first len(proof_files) rows the outputs that carry a proof
        (bound to `bindings` as verify_batch binds them; None: unbound); sum_start / entries / claims / key_start / keys as excess_sums_batch takes them
        (claims (amount, type, offset) per sum); msgs / sigs: one per key, as excess_verify_keys_batch takes them; offsets: the job positions of this
        shard's (proofs, keys, sums).  The combined point is V + K + S of the three calls under block_seeds(seed).  Returns accept, or (accept,
        (proof statuses, key statuses, sum statuses) or None, combined point or None) when want_status / want_point is set."""
        from .capi import RpBlock
        arrs, n = self.block_arrays(coms_files, proof_files, sum_start, entries, claims, key_start, keys, msgs, sigs, bindings)
        blk = RpBlock(proof_offset=offsets[0], key_offset=offsets[1], sum_offset=offsets[2], **n)
        dev = []
        try:
            for name, a in arrs:
                if a is None:
                    continue
                if _device:
                    dev.append(self.gpu.to_device(a))
                    setattr(blk, name, dev[-1])
                else:
                    setattr(blk, name, a.ctypes.data)
            return self.verify_block_call(blk, seed, want_status, want_point, device=_device)
        finally:
            for d in dev:
                self.gpu.free(d)

    def verify_block_device(self, *args, **kwargs):
        """bppp_rp_verify_block_device: verify_block with every buffer uploaded first (a caller whose buffers already lie in HBM fills a capi.RpBlock
        with the device pointers and calls verify_block_call(..., device=True))"""
        return self.verify_block(*args, _device=True, **kwargs)

    # ---- half-aggregate excess signatures: 33 bytes a kernel and one scalar (bppp_rp_excess_halfagg / _halfagg_verify, bppp_rp_verify_block_agg)
    def _excess_halfagg(self, fn, n, args, want_status):
        import ctypes as C
        import numpy as np
        status = np.zeros(max(n, 1), dtype=np.uint32)
        self.gpu._check(fn(self.h, *args, C.c_void_p(status.ctypes.data) if want_status else None), "bppp_rp_excess_halfagg")
        return [int(v) for v in status[:n]] if want_status else None

    def excess_halfagg(self, keys: Sequence[bytes], msgs: Sequence[bytes], sigs: Sequence[bytes], want_status: bool = False):
        """bppp_rp_excess_halfagg: the half-aggregate of the signatures, EXCESS_AGG_BYTES (n) bytes (b"" for no key): the R rows, then put (sum z_i s_i)
        with the coefficients of excess_halfagg_coef.  The equations are NOT evaluated: check the signatures first.  Returns the aggregate, or (aggregate,
        statuses) with want_status (all zero bytes when a signature is refused); without it a refusal raises BpppError."""
        import ctypes as C
        import numpy as np
        keep, n, args = self._excess_key_args(keys, msgs, sigs)
        ag = np.zeros(EXCESS_AGG_BYTES(n), dtype=np.uint8)
        st = self._excess_halfagg(self.gpu.lib.bppp_rp_excess_halfagg, n, args + (C.c_void_p(ag.ctypes.data),), want_status)
        out = ag.tobytes() if n else b""
        return (out, st) if want_status else out

    def excess_halfagg_device(self, nkeys: int, d_keys: int, d_msgs: int, d_sigs: int, d_agg: int, want_status: bool = False):
        """bppp_rp_excess_halfagg_device: excess_halfagg on buffers in HBM (d_agg receives EXCESS_AGG_BYTES (nkeys) bytes); returns the statuses or None"""
        import ctypes as C
        p = C.c_void_p
        return self._excess_halfagg(self.gpu.lib.bppp_rp_excess_halfagg_device, nkeys, (nkeys, p(d_keys), p(d_msgs), p(d_sigs), p(d_agg)), want_status)

    def _excess_halfagg_verify(self, fn, n, args, want_status, want_point):
        import ctypes as C
        import numpy as np
        from .capi import array_to_point
        acc, status, xy = C.c_int(0), np.zeros(max(n, 1), dtype=np.uint32), np.zeros(8, dtype=np.uint64)
        rc = fn(self.h, *args, C.byref(acc), C.c_void_p(status.ctypes.data) if want_status else None, C.c_void_p(xy.ctypes.data) if want_point else None)
        self.gpu._check(rc, "bppp_rp_excess_halfagg_verify")
        if not (want_status or want_point):
            return bool(acc.value)
        return bool(acc.value), ([int(v) for v in status[:n]] if want_status else None), (array_to_point(xy) if want_point else None)

    def excess_halfagg_verify(self, keys: Sequence[bytes], msgs: Sequence[bytes], agg: bytes, want_status: bool = False, want_point: bool = False):
        """bppp_rp_excess_halfagg_verify: does the half-aggregate hold for these keys and messages?  One equation, one MSM a pass and no seed.  Returns accept,
        or (accept, verdicts or None, the equation's left side or None) when want_status / want_point is set; the verdict of the equation is the same for
        every key it is asked of: an aggregate cannot name a culprit."""
        import ctypes as C
        import numpy as np
        n = len(keys)
        if len(msgs) != n or len(agg) != (EXCESS_AGG_BYTES(n) if n else len(agg)):
            raise ValueError("one message per key and an aggregate of 33 n + 32 bytes are required")
        keep = [self._excess_bytes(keys, EXCESS_KEY_BYTES, "keys"), self._excess_bytes(msgs, 32, "messages"), np.frombuffer(agg or b"\0", dtype=np.uint8)]
        return self._excess_halfagg_verify(self.gpu.lib.bppp_rp_excess_halfagg_verify, n, (n,) + tuple(C.c_void_p(a.ctypes.data) for a in keep), want_status, want_point)

    def excess_halfagg_verify_device(self, nkeys: int, d_keys: int, d_msgs: int, d_agg: int, want_status: bool = False, want_point: bool = False):
        """bppp_rp_excess_halfagg_verify_device: excess_halfagg_verify on buffers in HBM"""
        import ctypes as C
        p = C.c_void_p
        return self._excess_halfagg_verify(self.gpu.lib.bppp_rp_excess_halfagg_verify_device, nkeys, (nkeys, p(d_keys), p(d_msgs), p(d_agg)), want_status, want_point)

    def verify_block_agg(self, coms_files: Sequence[bytes], proof_files: Sequence[bytes], sum_start, entries, claims, key_start, keys: Sequence[bytes], msgs: Sequence[bytes],
                         agg: bytes, bindings=None, seed: Optional[bytes] = None, offsets=(0, 0, 0), want_status: bool = False, want_point: bool = False,
                         _device: bool = False):
        """bppp_rp_verify_block_agg: verify_block with the half-aggregate of the kernel signatures (excess_halfagg) in their place: the combined point is
        V + K' + S with K' = block_agg_weight (...) times the point of excess_halfagg_verify.  offsets: (proofs, keys, sums); the keys' must be 0, an
        aggregate is not shardable.  Returns as verify_block does; on rejection the key statuses are those of excess_halfagg_verify."""
        import numpy as np
        from .capi import RpBlock
        nkeys = len(keys)
        if len(agg) != (EXCESS_AGG_BYTES(nkeys) if nkeys else len(agg)):
            raise ValueError("an aggregate of 33 nkeys + 32 bytes is required")
        arrs, n = self.block_arrays(coms_files, proof_files, sum_start, entries, claims, key_start, keys, msgs, [bytes(EXCESS_SIG_BYTES)] * nkeys, bindings)
        arrs = [(name, a) for name, a in arrs if name != "sigs"] + [("agg", np.frombuffer(agg or b"\0", dtype=np.uint8))]
        blk = RpBlock(proof_offset=offsets[0], key_offset=offsets[1], sum_offset=offsets[2], **n)
        dev, at = [], {}
        try:
            for name, a in arrs:
                if a is None:
                    continue
                if _device:
                    dev.append(self.gpu.to_device(a))
                at[name] = dev[-1] if _device else a.ctypes.data
                if name != "agg":
                    setattr(blk, name, at[name])
            return self.verify_block_call(blk, seed, want_status, want_point, device=_device, agg=at["agg"])
        finally:
            for d in dev:
                self.gpu.free(d)

    def verify_block_agg_device(self, *args, **kwargs):
        """bppp_rp_verify_block_agg_device: verify_block_agg with every buffer uploaded first"""
        return self.verify_block_agg(*args, _device=True, **kwargs)

    # ---- the multi-party signer: parties who each know a part of the blinding sum (bppp_rp_excess_part_nonces / _aggregate / _sign / _verify / _combine)
    def _excess_part_rows(self, fn, name, n, args, out_specs, want_status, status_len=None):
        """one builder call: args before the outputs; out_specs [(row bytes, rows, wanted)]; returns (outputs as row lists or None, statuses or None)"""
        import ctypes as C
        import numpy as np
        bufs = [np.zeros(max(rows, 1) * width, dtype=np.uint8) if wanted else None for width, rows, wanted in out_specs]
        status = np.zeros(max(status_len if status_len is not None else n, 1), dtype=np.uint32)
        vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        self.gpu._check(fn(self.h, *args, *[vp(b) for b in bufs], vp(status) if want_status else None), name)
        outs = []
        for (width, rows, wanted), b in zip(out_specs, bufs):
            raw = b.tobytes() if wanted else None
            outs.append([raw[t * width:(t + 1) * width] for t in range(rows)] if wanted else None)
        return outs, ([int(v) for v in status[:status_len if status_len is not None else n]] if want_status else None)

    def _excess_part_device(self, fn, name, args, n_status, want_status):
        import ctypes as C
        import numpy as np
        status = np.zeros(max(n_status, 1), dtype=np.uint32)
        self.gpu._check(fn(self.h, *args, C.c_void_p(status.ctypes.data) if want_status else None), name)
        return [int(v) for v in status[:n_status]] if want_status else None

    def excess_part_nonces(self, blinds: Sequence[int], msgs: Sequence[bytes], aux: bytes, want_status: bool = False):
        """bppp_rp_excess_part_nonces: round 1 of one party for len(blinds) sessions.  Returns the 66-byte public nonces, or (nonces, statuses) with
        want_status (a refused row has zero bytes); without it a refused row raises BpppError.  aux: 32 bytes of fresh randomness."""
        import ctypes as C
        import numpy as np
        from .capi import scalars_to_array
        n = len(blinds)
        if len(msgs) != n or len(aux) != 32:
            raise ValueError("one 32-byte message per session and 32 bytes of aux are required")
        bl, mg, ax = scalars_to_array(list(blinds) or [0]), self._excess_bytes(msgs, 32, "messages"), np.frombuffer(aux, dtype=np.uint8)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        (out,), st = self._excess_part_rows(self.gpu.lib.bppp_rp_excess_part_nonces, "bppp_rp_excess_part_nonces", n, (n, vp(bl), vp(mg), vp(ax)),
                                            [(EXCESS_PUBNONCE_BYTES, n, True)], want_status)
        return (out, st) if want_status else out

    def excess_part_nonces_device(self, n: int, d_blinds: int, d_msgs: int, d_pubnonces: int, aux: bytes, want_status: bool = False):
        """bppp_rp_excess_part_nonces_device: excess_part_nonces on buffers in HBM (d_pubnonces receives [n][66] bytes); returns the statuses or None"""
        import ctypes as C
        import numpy as np
        p, ax = C.c_void_p, np.frombuffer(aux, dtype=np.uint8)
        return self._excess_part_device(self.gpu.lib.bppp_rp_excess_part_nonces_device, "bppp_rp_excess_part_nonces", (n, p(d_blinds), p(d_msgs), p(ax.ctypes.data), p(d_pubnonces)),
                                        n, want_status)

    def _excess_part_groups(self, part_start, pubnonces, keys, partials=None, msgs=None):
        import ctypes as C
        import numpy as np
        nsums, nparts = len(part_start) - 1, len(pubnonces)
        if len(keys) != nparts or (partials is not None and len(partials) != nparts) or (msgs is not None and len(msgs) != nsums):
            raise ValueError("one public nonce, one key and one partial per part and one message per sum are required")
        keep = [np.array(list(part_start), dtype=np.uint32), self._excess_bytes(pubnonces, EXCESS_PUBNONCE_BYTES, "public nonces"), self._excess_bytes(keys, EXCESS_KEY_BYTES, "keys")]
        if partials is not None:
            keep += [self._excess_bytes(partials, EXCESS_PARTIAL_BYTES, "partials"), self._excess_bytes(msgs, 32, "messages")]
        return keep, nsums, nparts, (nsums, nparts) + tuple(C.c_void_p(a.ctypes.data) for a in keep)

    def excess_part_aggregate(self, part_start, pubnonces: Sequence[bytes], keys: Sequence[bytes], want_status: bool = False):
        """bppp_rp_excess_part_aggregate: the coordinator's step; the parts of sum t are rows part_start[t] .. part_start[t + 1].  Returns (aggregated nonces
        of 66 bytes, aggregated keys of 33 bytes), with the statuses as a third component with want_status; without it a refused sum raises BpppError."""
        keep, nsums, nparts, args = self._excess_part_groups(part_start, pubnonces, keys)
        (an, ak), st = self._excess_part_rows(self.gpu.lib.bppp_rp_excess_part_aggregate, "bppp_rp_excess_part_aggregate", nsums, args,
                                              [(EXCESS_PUBNONCE_BYTES, nsums, True), (EXCESS_KEY_BYTES, nsums, True)], want_status)
        return (an, ak, st) if want_status else (an, ak)

    def excess_part_aggregate_device(self, nsums: int, nparts: int, d_part_start: int, d_pubnonces: int, d_keys: int, d_agg_nonces: int, d_agg_keys: int, want_status: bool = False):
        """bppp_rp_excess_part_aggregate_device: excess_part_aggregate on buffers in HBM; returns the statuses or None"""
        import ctypes as C
        p = C.c_void_p
        return self._excess_part_device(self.gpu.lib.bppp_rp_excess_part_aggregate_device, "bppp_rp_excess_part_aggregate",
                                        (nsums, nparts, p(d_part_start), p(d_pubnonces), p(d_keys), p(d_agg_nonces), p(d_agg_keys)), nsums, want_status)

    def excess_part_sign(self, blinds: Sequence[int], msgs: Sequence[bytes], aux: bytes, agg_nonces: Sequence[bytes], agg_keys: Sequence[bytes], want_status: bool = False):
        """bppp_rp_excess_part_sign: round 2 of one party: the 32-byte partial responses, or (partials, statuses) with want_status.  aux is the aux of round 1;
        never sign twice with one (blinding, message, aux) under different aggregates."""
        import ctypes as C
        import numpy as np
        from .capi import scalars_to_array
        n = len(blinds)
        if len(msgs) != n or len(agg_nonces) != n or len(agg_keys) != n or len(aux) != 32:
            raise ValueError("one message, one aggregated nonce and one aggregated key per session and 32 bytes of aux are required")
        keep = [scalars_to_array(list(blinds) or [0]), self._excess_bytes(msgs, 32, "messages"), np.frombuffer(aux, dtype=np.uint8),
                self._excess_bytes(agg_nonces, EXCESS_PUBNONCE_BYTES, "aggregated nonces"), self._excess_bytes(agg_keys, EXCESS_KEY_BYTES, "aggregated keys")]
        (out,), st = self._excess_part_rows(self.gpu.lib.bppp_rp_excess_part_sign, "bppp_rp_excess_part_sign", n, (n,) + tuple(C.c_void_p(a.ctypes.data) for a in keep),
                                            [(EXCESS_PARTIAL_BYTES, n, True)], want_status)
        return (out, st) if want_status else out

    def excess_part_sign_device(self, n: int, d_blinds: int, d_msgs: int, d_agg_nonces: int, d_agg_keys: int, d_partials: int, aux: bytes, want_status: bool = False):
        """bppp_rp_excess_part_sign_device: excess_part_sign on buffers in HBM (d_partials receives [n][32] bytes); returns the statuses or None"""
        import ctypes as C
        import numpy as np
        p, ax = C.c_void_p, np.frombuffer(aux, dtype=np.uint8)
        return self._excess_part_device(self.gpu.lib.bppp_rp_excess_part_sign_device, "bppp_rp_excess_part_sign",
                                        (n, p(d_blinds), p(d_msgs), p(ax.ctypes.data), p(d_agg_nonces), p(d_agg_keys), p(d_partials)), n, want_status)

    def _excess_part_verify(self, fn, nsums, nparts, args):
        import ctypes as C
        import numpy as np
        status, sst = np.zeros(max(nparts, 1), dtype=np.uint32), np.zeros(max(nsums, 1), dtype=np.uint32)
        self.gpu._check(fn(self.h, *args, C.c_void_p(status.ctypes.data), C.c_void_p(sst.ctypes.data)), "bppp_rp_excess_part_verify")
        return [int(v) for v in status[:nparts]], [int(v) for v in sst[:nsums]]

    def excess_part_verify(self, part_start, pubnonces: Sequence[bytes], keys: Sequence[bytes], partials: Sequence[bytes], msgs: Sequence[bytes]):
        """bppp_rp_excess_part_verify: who misbehaved: (one verdict per part, one verdict per sum)"""
        keep, nsums, nparts, args = self._excess_part_groups(part_start, pubnonces, keys, partials, msgs)
        return self._excess_part_verify(self.gpu.lib.bppp_rp_excess_part_verify, nsums, nparts, args)

    def excess_part_verify_device(self, nsums: int, nparts: int, d_part_start: int, d_pubnonces: int, d_keys: int, d_partials: int, d_msgs: int):
        """bppp_rp_excess_part_verify_device: excess_part_verify on buffers in HBM"""
        import ctypes as C
        p = C.c_void_p
        return self._excess_part_verify(self.gpu.lib.bppp_rp_excess_part_verify_device, nsums, nparts,
                                        (nsums, nparts, p(d_part_start), p(d_pubnonces), p(d_keys), p(d_partials), p(d_msgs)))

    def excess_part_combine(self, part_start, pubnonces: Sequence[bytes], keys: Sequence[bytes], partials: Sequence[bytes], msgs: Sequence[bytes], want_status: bool = False,
                            want_keys: bool = False):
        """bppp_rp_excess_part_combine: the 65-byte signatures, or (signatures, statuses or None, aggregated keys or None) as asked; the partials are not
        checked — verify the signature under the aggregated key, and ask excess_part_verify only when that fails"""
        keep, nsums, nparts, args = self._excess_part_groups(part_start, pubnonces, keys, partials, msgs)
        (sg, ak), st = self._excess_part_rows(self.gpu.lib.bppp_rp_excess_part_combine, "bppp_rp_excess_part_combine", nsums, args,
                                              [(EXCESS_SIG_BYTES, nsums, True), (EXCESS_KEY_BYTES, nsums, want_keys)], want_status)
        return (sg, st, ak) if (want_status or want_keys) else sg

    def excess_part_combine_device(self, nsums: int, nparts: int, d_part_start: int, d_pubnonces: int, d_keys: int, d_partials: int, d_msgs: int, d_sigs: int, d_agg_keys: int = 0,
                                   want_status: bool = False):
        """bppp_rp_excess_part_combine_device: excess_part_combine on buffers in HBM (d_agg_keys 0: not wanted); returns the statuses or None"""
        import ctypes as C
        p = C.c_void_p
        return self._excess_part_device(self.gpu.lib.bppp_rp_excess_part_combine_device, "bppp_rp_excess_part_combine",
                                        (nsums, nparts, p(d_part_start), p(d_pubnonces), p(d_keys), p(d_partials), p(d_msgs), p(d_sigs), p(d_agg_keys or None)), nsums, want_status)

    def share_comb(self, donor: "NativeRangeProofs"):
        """bppp_rp_share_comb: prove over `donor`'s comb table from now on (built now if it has none).  Same context; the donor's basis
        must extend this handle's point by point.  The table lives until its last user is closed."""
        self.gpu._check(self.gpu.lib.bppp_rp_share_comb(self.h, donor.h), "bppp_rp_share_comb")

    def comb_info(self) -> dict:
        """bppp_rp_comb_info: window_bits, bytes, points and users of the comb table this handle proves over (all 0 without one)"""
        import ctypes as C
        c, nb, npt, nu = C.c_int(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self.gpu._check(self.gpu.lib.bppp_rp_comb_info(self.h, C.byref(c), C.byref(nb), C.byref(npt), C.byref(nu)), "bppp_rp_comb_info")
        return {"window_bits": int(c.value), "bytes": int(nb.value), "points": int(npt.value), "users": int(nu.value)}

    def verify_batch(self, coms_files: Sequence[bytes], proof_files: Sequence[bytes], seed: Optional[bytes] = None, want_status: bool = False,
                     want_challenges: bool = False, public_amounts=None, bindings=None):
        """bppp_rp_verify_batch on host byte strings: returns accept, or (accept, status list, challenges per proof) as asked.
        `seed` is the verifier's randomness behind the batch weights: fresh from os.urandom unless given (fixed seeds are for tests).
        public_amounts: per-proof public amounts as for prove_batch (bppp_rp_verify_batch_pub), taken from the transactions.
        bindings: per-proof 32-byte bindings as for prove_batch (bppp_rp_verify_bound), derived from the transactions, never taken from the prover."""
        import ctypes as C
        import numpy as np
        from .capi import bindings_array
        if seed is None:
            seed = os.urandom(32)
        B = len(proof_files)
        bindings_array(bindings, B)
        if len(coms_files) != B or len(seed) != 32:
            raise ValueError("one commitments file per proof and a 32-byte seed are required")
        if any(len(c) != self.shape["coms_bytes"] for c in coms_files) or any(len(p_) != self.shape["proof_bytes"] for p_ in proof_files):
            return (False, [2] * B, None) if (want_status or want_challenges) else False       # wrong length: malformed, as decodeProof' returns Nothing
        cb, pb = np.frombuffer(b"".join(coms_files), dtype=np.uint8), np.frombuffer(b"".join(proof_files), dtype=np.uint8)
        with self._public_arg(public_amounts, B, False) as pa:
            if bindings is None:
                return self._verify(self.gpu.lib.bppp_rp_verify_batch_pub, B, C.c_void_p(cb.ctypes.data), C.c_void_p(pb.ctypes.data), pa, seed, want_status, want_challenges)
            with self._bindings_arg(bindings, B, False) as ba:
                fn = lambda h, n, pc, pp, pa_, *rest: self.gpu.lib.bppp_rp_verify_bound(h, n, pc, pp, pa_, ba, *rest)
                return self._verify(fn, B, C.c_void_p(cb.ctypes.data), C.c_void_p(pb.ctypes.data), pa, seed, want_status, want_challenges)

    def verify_batch_device(self, batch: int, d_coms: int, d_proofs: int, seed: Optional[bytes] = None, want_status: bool = False, want_challenges: bool = False,
                            public_amounts=None, bindings=None):
        """bppp_rp_verify_batch_device; public_amounts: per-proof values (uploaded for the call) or a device pointer to the
        [batch][public_count][4] words (bppp_rp_verify_batch_pub_device); bindings: per-proof values (uploaded for the call) or a device
        pointer to the [batch][32] bytes (bppp_rp_verify_bound_device)"""
        import ctypes as C
        if seed is None:
            seed = os.urandom(32)
        with self._public_arg(public_amounts, batch, True) as pa:
            if bindings is None:
                return self._verify(self.gpu.lib.bppp_rp_verify_batch_pub_device, batch, C.c_void_p(d_coms), C.c_void_p(d_proofs), pa, seed, want_status, want_challenges)
            with self._bindings_arg(bindings, batch, True) as ba:
                fn = lambda h, n, pc, pp, pa_, *rest: self.gpu.lib.bppp_rp_verify_bound_device(h, n, 0, pc, pp, pa_, ba, *rest)
                return self._verify(fn, batch, C.c_void_p(d_coms), C.c_void_p(d_proofs), pa, seed, want_status, want_challenges)

    def verify_batch_device_point(self, batch: int, d_coms: int, d_proofs: int, seed: bytes, index_offset: int = 0, public_amounts=None, bindings=None) -> Tuple[bool, Point]:
        """bppp_rp_verify_shard_device: (accept, the combined point) — the partial result of one rank when the job is sharded
        proof-per-GPU; this rank holds proofs [index_offset, index_offset + batch) of the job, every rank passes the same seed.
        public_amounts as for verify_batch_device (bppp_rp_verify_shard_pub_device); bindings as there, those of this rank's own proofs
        (bppp_rp_verify_bound_device)."""
        import ctypes as C
        import numpy as np
        from .capi import array_to_point
        acc, out = C.c_int(0), np.zeros(8, dtype=np.uint64)
        sd = np.frombuffer(seed, dtype=np.uint8)
        with self._public_arg(public_amounts, batch, True) as pa:
            if bindings is None:
                rc = self.gpu.lib.bppp_rp_verify_shard_pub_device(self.h, batch, index_offset, C.c_void_p(d_coms), C.c_void_p(d_proofs), pa, C.c_void_p(sd.ctypes.data),
                                                                  C.byref(acc), None, None, C.c_void_p(out.ctypes.data))
            else:
                with self._bindings_arg(bindings, batch, True) as ba:
                    rc = self.gpu.lib.bppp_rp_verify_bound_device(self.h, batch, index_offset, C.c_void_p(d_coms), C.c_void_p(d_proofs), pa, ba, C.c_void_p(sd.ctypes.data),
                                                                  C.byref(acc), None, None, C.c_void_p(out.ctypes.data))
        self.gpu._check(rc, "bppp_rp_verify_shard_device")
        return bool(acc.value), array_to_point(out)

    def verify_each(self, coms_files: Sequence[bytes], proof_files: Sequence[bytes], want_points: bool = False, public_amounts=None, bindings=None):
        """bppp_rp_verify_each on host byte strings: every proof decided on its own, without weights or seed.  Returns the status list
        (0 valid, 1 invalid, 2 malformed), or (statuses, [E_b per proof]) with want_points (None for infinity, and for a malformed
        proof).  A file of the wrong length makes the whole batch MALFORMED without a library call, as verify_batch does.
        public_amounts and bindings as for verify_batch (bppp_rp_verify_each_pub, bppp_rp_verify_each_bound)."""
        import ctypes as C
        import numpy as np
        from .capi import bindings_array
        B = len(proof_files)
        bindings_array(bindings, B)
        if len(coms_files) != B:
            raise ValueError("one commitments file per proof is required")
        if any(len(c) != self.shape["coms_bytes"] for c in coms_files) or any(len(p_) != self.shape["proof_bytes"] for p_ in proof_files):
            return ([2] * B, [None] * B) if want_points else [2] * B
        cb = np.frombuffer(b"".join(coms_files) or b"\0", dtype=np.uint8)
        pb = np.frombuffer(b"".join(proof_files) or b"\0", dtype=np.uint8)
        with self._public_arg(public_amounts, B, False) as pa:
            if bindings is None:
                return self._verify_each(self.gpu.lib.bppp_rp_verify_each_pub, B, C.c_void_p(cb.ctypes.data), C.c_void_p(pb.ctypes.data), pa, want_points)
            with self._bindings_arg(bindings, B, False) as ba:
                fn = lambda h, n, pc, pp, pa_, *rest: self.gpu.lib.bppp_rp_verify_each_bound(h, n, pc, pp, pa_, ba, *rest)
                return self._verify_each(fn, B, C.c_void_p(cb.ctypes.data), C.c_void_p(pb.ctypes.data), pa, want_points)

    def verify_each_device(self, batch: int, d_coms: int, d_proofs: int, want_points: bool = False, public_amounts=None, bindings=None):
        """bppp_rp_verify_each_device: verify_each on files already in HBM (device pointers); public_amounts and bindings as for verify_batch_device"""
        import ctypes as C
        with self._public_arg(public_amounts, batch, True) as pa:
            if bindings is None:
                return self._verify_each(self.gpu.lib.bppp_rp_verify_each_pub_device, batch, C.c_void_p(d_coms), C.c_void_p(d_proofs), pa, want_points)
            with self._bindings_arg(bindings, batch, True) as ba:
                fn = lambda h, n, pc, pp, pa_, *rest: self.gpu.lib.bppp_rp_verify_each_bound_device(h, n, pc, pp, pa_, ba, *rest)
                return self._verify_each(fn, batch, C.c_void_p(d_coms), C.c_void_p(d_proofs), pa, want_points)

    def _verify_each(self, fn, B, pc, pp, pa, want_points):
        import ctypes as C
        import numpy as np
        from .capi import array_to_point
        status = np.zeros(max(B, 1), dtype=np.uint32)
        xy = np.zeros((max(B, 1), 8), dtype=np.uint64) if want_points else None
        rc = fn(self.h, B, pc, pp, pa, C.c_void_p(status.ctypes.data), C.c_void_p(xy.ctypes.data) if want_points else None)
        self.gpu._check(rc, "bppp_rp_verify_each")
        st = [int(v) for v in status[:B]]
        return (st, [array_to_point(xy[b]) for b in range(B)]) if want_points else st

    def _verify(self, fn, B, pc, pp, pa, seed, want_status, want_challenges):
        import ctypes as C
        import numpy as np
        from .capi import array_to_scalars
        acc = C.c_int(0)
        status = np.zeros(max(B, 1), dtype=np.uint32) if want_status else None
        nch = self.shape["challenges_per_proof"]
        chal = np.zeros((max(B, 1) * nch, 4), dtype=np.uint64) if want_challenges else None
        sd = np.frombuffer(seed, dtype=np.uint8)
        rc = fn(self.h, B, pc, pp, pa, C.c_void_p(sd.ctypes.data), C.byref(acc), C.c_void_p(status.ctypes.data) if want_status else None,
                C.c_void_p(chal.ctypes.data) if want_challenges else None, None)
        self.gpu._check(rc, "bppp_rp_verify_batch")
        if not (want_status or want_challenges):
            return bool(acc.value)
        chs = None
        if want_challenges:
            flat = array_to_scalars(chal)
            lead = nch - self.shape["rounds"]               # 7 range-proof challenges (typed reciprocal) or 4 (binary), then one per round
            chs = [(flat[b * nch:b * nch + lead], flat[b * nch + lead:(b + 1) * nch]) for b in range(B)]
        return bool(acc.value), ([int(v) for v in status[:B]] if want_status else None), chs


def open_weight(seed: bytes, j: int, x: bytes, sign: int, v: int, ty: int, bl: int) -> int:
    """The weight rho_j bppp_rp_open_batch gives the opening at job position j (include/bppp.h states the message): x = the commitment's 32
    x bytes as they stand in the file, sign = its sign bit, (v, ty, bl) the claimed scalars (v already reduced mod N; ty = 0 on a binary handle)."""
    put = lambda s: b"".join(((s >> (64 * i)) & (2**64 - 1)).to_bytes(8, "big") for i in range(4))      # Binary (Prime p) put (Encoding.hs:81-86)
    msg = seed + (j % 2**64).to_bytes(8, "little") + x + bytes([sign]) + put(v) + put(ty) + put(bl)
    return decode_field(hashlib.sha256(msg).digest(), N) or 1


TALLY_SUBTRACT = 1 << 31


def tally_entry(j: int, subtract: bool = False) -> int:
    """one entry of a tally's CSR: the flat index j = row * nranges + i of a commitment, bit 31 set when it is subtracted"""
    if not 0 <= j < TALLY_SUBTRACT:
        raise ValueError("a flat index is below 2^31")
    return j | (TALLY_SUBTRACT if subtract else 0)


def tally_amount_word(a: int) -> int:
    """the 256-bit two's-complement word that names the amount a mod N to the entry points: the residue when it is below 2^255, else the residue - N"""
    r = a % N
    return r if r < 2**255 else (r - N) % 2**256


def tally_weight(seed: bytes, t: int, a: int, ty: int, e: int) -> int:
    """The weight rho_t bppp_rp_tally_batch gives the sum at job position t (include/bppp.h states the message): (a, ty, e) the claim, a
    already reduced mod N; ty = 0 on a binary handle.  The pool and the entries are not in the message: they are the checker's own inputs."""
    put = lambda s: b"".join(((s >> (64 * i)) & (2**64 - 1)).to_bytes(8, "big") for i in range(4))      # Binary (Prime p) put (Encoding.hs:81-86)
    msg = seed + (t % 2**64).to_bytes(8, "little") + put(a) + put(ty) + put(e)
    return decode_field(hashlib.sha256(msg).digest(), N) or 1


def tally_sums(backend: "Backend", points: Sequence[Point], sum_start: Sequence[int], entries: Sequence[int]) -> List[Point]:
    """Host restatement of the segmented signed sum over the Backend group operations: S_t = sum over entries [sum_start[t], sum_start[t + 1])
    of +-points[index]; None is the identity (an empty sum, or one that cancels)."""
    out = []
    for t in range(len(sum_start) - 1):
        es = entries[sum_start[t]:sum_start[t + 1]]
        out.append(backend.commit([N - 1 if e & TALLY_SUBTRACT else 1 for e in es], [points[e & (TALLY_SUBTRACT - 1)] for e in es]) if es else None)
    return out


def tally_claims_host(triples: Sequence[Tuple[int, int, int]], sum_start: Sequence[int], entries: Sequence[int]) -> List[Tuple[int, int, int]]:
    """Host restatement of bppp_rp_tally_claims: triples[j] = (amount, type, blinding) of the commitment with flat index j (amounts any
    integers, negative ones too); one (a, ty, e) mod N per sum."""
    out = []
    for t in range(len(sum_start) - 1):
        acc = [0, 0, 0]
        for e in entries[sum_start[t]:sum_start[t + 1]]:
            sign = -1 if e & TALLY_SUBTRACT else 1
            for k in range(3):
                acc[k] += sign * triples[e & (TALLY_SUBTRACT - 1)][k]
        out.append(tuple(v % N for v in acc))
    return out


# ----------------------------------------------------------------------------- cut-through (bppp_rp_cut_through; include/bppp.h states every rule)
CUT_KEPT, CUT_SPENT, CUT_KEPT_AGAIN = 0, 1, 2


@dataclass
class CutThrough:
    """what bppp_rp_cut_through returns: the new pool, the surviving entries re-based to it (the block's one sum), row_map[k] = the old index of new
    row k, out_rows = how many of the new rows are new outputs (they stand in front), one CUT_* per entry of the job, the summed claim (None without
    claims) and the counts of bppp_rp_cut_counts as a dict"""
    coms_files: List[bytes]
    entries: List[int]
    row_map: List[int]
    out_rows: int
    entry_status: List[int]
    claims: Optional[tuple]
    counts: Dict[str, int]


def cut_identity(nranges: int, coms_file: bytes, i: int) -> Tuple[int, int]:
    """the identity of commitment i of a commitments file: (x mod p, bit i of the sign bytes) — the 33 bytes put (x mod p) || sign as a pair"""
    o = (nranges + 7) // 8 + 32 * i
    return decode_field(coms_file[o:o + 32], FIELD_P), (coms_file[i >> 3] >> (i & 7)) & 1


def cut_through_host(nranges: int, coms_files: Sequence[bytes], sum_start: Sequence[int], entries: Sequence[int], claims=None) -> CutThrough:
    """Host restatement of bppp_rp_cut_through with dictionaries and lists: no GPU, no backend, no curve.  claims: None, or one (amount, type, offset)
    per sum ((amount, offset) for a binary handle) — amounts any integers, types and offsets below N (ValueError otherwise, the call's BPPP_ERR_ARG)."""
    nsums, nnz, rows = len(sum_start) - 1, len(entries), len(coms_files)
    zero = dict(new_rows=0, out_rows=0, new_nnz=0, ncut=0, nagain=0)
    width = len(claims[0]) if claims else 3
    if nsums <= 0 or nnz == 0:
        return CutThrough([], [], [], 0, [], None if claims is None else (0,) * width, zero)
    if list(sum_start) != sorted(sum_start) or sum_start[0] != 0 or sum_start[-1] != nnz:
        raise ValueError("sum_start is not non-decreasing from 0 to nnz")
    if any((e & (TALLY_SUBTRACT - 1)) >= rows * nranges for e in entries):
        raise ValueError("an entry's index is not below rows * nranges")
    block = None
    if claims is not None:
        if len(claims) != nsums:
            raise ValueError("one claim per sum is required")
        for t, c in enumerate(claims):
            if any(not 0 <= v < N for v in c[1:]):
                raise ValueError(f"sum {t}: a claimed type or offset is not canonical (>= n)")
        block = tuple(sum(c[k] for c in claims) % N for k in range(width))
    ident = [cut_identity(nranges, coms_files[(e & (TALLY_SUBTRACT - 1)) // nranges], (e & (TALLY_SUBTRACT - 1)) % nranges) for e in entries]
    count: Dict[tuple, List[int]] = {}
    for e, idt in zip(entries, ident):
        count.setdefault(idt, [0, 0])[e >> 31] += 1
    seen: Dict[tuple, List[int]] = {}
    status = []
    for e, idt in zip(entries, ident):
        rank = seen.setdefault(idt, [0, 0])
        m = min(count[idt])
        status.append(CUT_SPENT if rank[e >> 31] < m else CUT_KEPT if rank[e >> 31] == m else CUT_KEPT_AGAIN)
        rank[e >> 31] += 1
    kept = [e for e, s in zip(entries, status) if s != CUT_SPENT]
    outs = sorted({(e & (TALLY_SUBTRACT - 1)) // nranges for e in kept if not e & TALLY_SUBTRACT})
    rest = sorted({(e & (TALLY_SUBTRACT - 1)) // nranges for e in kept} - set(outs))
    row_map = outs + rest
    new_of = {r: k for k, r in enumerate(row_map)}
    new_entries = [(e & TALLY_SUBTRACT) | (new_of[(e & (TALLY_SUBTRACT - 1)) // nranges] * nranges + (e & (TALLY_SUBTRACT - 1)) % nranges) for e in kept]
    counts = dict(new_rows=len(row_map), out_rows=len(outs), new_nnz=len(kept), ncut=status.count(CUT_SPENT), nagain=status.count(CUT_KEPT_AGAIN))
    return CutThrough([bytes(coms_files[r]) for r in row_map], new_entries, row_map, len(outs), status, block, counts)


# ----------------------------------------------------------------------------- excess signatures (bppp_rp_excess_*; include/bppp.h states every message)
def block_seeds(seed: bytes) -> Tuple[bytes, bytes, bytes]:
    """the part seeds of bppp_rp_verify_block: SHA-256 (b"bppp block" + seed + bytes([p])) for p = 0 (proofs), 1 (signatures), 2 (sums)"""
    if len(seed) != 32:
        raise ValueError("a 32-byte seed is required")
    return tuple(hashlib.sha256(b"bppp block" + seed + bytes([p])).digest() for p in range(3))


FIELD_P = 2**256 - 2**32 - 977
EXCESS_SIG_BYTES = 65
EXCESS_OK, EXCESS_NOT_CANONICAL, EXCESS_ZERO, EXCESS_NONCE, EXCESS_BAD_R, EXCESS_NO_KEY = 0, 1, 2, 3, 4, 5
EXCESS_KEY_BYTES = 33
EXCESS_BAD_KEY = 6


def _put(s: int) -> bytes:
    """Binary (Prime p) put (Encoding.hs:81-86): the four 64-bit limbs least significant first, each big-endian"""
    return b"".join(((s >> (64 * i)) & (2**64 - 1)).to_bytes(8, "big") for i in range(4))


def _point33(p: Tuple[int, int]) -> bytes:
    """put (x) and the sign byte (y > p - y) of an affine point"""
    return _put(p[0]) + bytes([1 if p[1] > FIELD_P - p[1] else 0])


def excess_nonce(tag: bytes, e: int, msg: bytes, aux: bytes) -> int:
    """k = decode (SHA-256 (Dn || put (e) || msg || aux)) mod n, Dn = SHA-256 ("bppp/excess/nonce/v1" || tag): 128 bytes"""
    return decode_field(hashlib.sha256(hashlib.sha256(b"bppp/excess/nonce/v1" + tag).digest() + _put(e) + msg + aux).digest(), N)


def excess_challenge(tag: bytes, r33: bytes, X: Tuple[int, int], msg: bytes) -> int:
    """c = decode (SHA-256 (Dc || the 33 bytes of R as the signature holds them || put (X.x) || sign (X) || msg)) mod n,
    Dc = SHA-256 ("bppp/excess/challenge/v1" || tag): 130 bytes"""
    return decode_field(hashlib.sha256(hashlib.sha256(b"bppp/excess/challenge/v1" + tag).digest() + r33 + _point33(X) + msg).digest(), N)


def excess_weight(seed: bytes, t: int, sig: bytes, X: Tuple[int, int], msg: bytes) -> int:
    """rho_t of bppp_rp_excess_verify_batch: decode (SHA-256 (seed || le64 (t) || sig[65] || put (X.x) || sign (X) || msg)) mod n, 1 for 0: 170 bytes"""
    return decode_field(hashlib.sha256(seed + (t % 2**64).to_bytes(8, "little") + sig + _point33(X) + msg).digest(), N) or 1


def _excess_bases(setup):
    """(g, H0 or None, B): B = H1 of a typed setup, h0 of a binary one (which has no type base)"""
    return (setup.g, setup.hs[0], setup.hs[1]) if isinstance(setup, SetupTRRP) else (setup.g, None, setup.hs[0])


def _commit_terms(backend: "Backend", terms) -> Point:
    terms = [(s % N, p) for s, p in terms if p is not None and s % N]
    return backend.commit([s for s, _ in terms], [p for _, p in terms]) if terms else None


def excess_sign_host(backend: "Backend", setup, e: int, msg: bytes, aux: bytes, tag: bytes = b""):
    """Host restatement of bppp_rp_excess_sign for one sum: (status, the 65 signature bytes, X = e B); a refused sum has zero bytes and no point"""
    _, _, B = _excess_bases(setup)
    status = EXCESS_NOT_CANONICAL if not 0 <= e < N else EXCESS_ZERO if e == 0 else EXCESS_OK
    k = excess_nonce(tag, e, msg, aux) if status == EXCESS_OK else 0
    if status == EXCESS_OK and k == 0:
        status = EXCESS_NONCE
    if status != EXCESS_OK:
        return status, bytes(EXCESS_SIG_BYTES), None
    R, X = backend.commit([k], [B]), backend.commit([e], [B])
    r33 = _point33(R)
    return status, r33 + _put((k + excess_challenge(tag, r33, X, msg) * e) % N), X


def excess_key_host(backend: "Backend", setup, S: Point, claim) -> Point:
    """X = S - a g - ty H0 (a binary setup: S - a g); claim = (a, ty, ...) typed, (a, ...) binary"""
    g, H0, _ = _excess_bases(setup)
    return _commit_terms(backend, [(1, S), (-claim[0], g)] + ([(-claim[1], H0)] if H0 is not None else []))


def excess_verify_host(backend: "Backend", setup, S: Point, claim, msg: bytes, sig: bytes, tag: bytes = b"", malformed: bool = False) -> int:
    """Host restatement of bppp_rp_excess_verify_each for one sum S (None: the identity; malformed: some referenced x has no curve point):
    the first verdict that applies, in the header's order"""
    _, H0, B = _excess_bases(setup)
    if malformed:
        return 2
    s = sum(int.from_bytes(sig[33 + 8 * i:41 + 8 * i], "big") << (64 * i) for i in range(4))
    if (H0 is not None and not 0 <= claim[1] < N) or s >= N:
        return 3
    x = decode_field(sig[:32], FIELD_P)
    y = pow((x * x * x + 7) % FIELD_P, (FIELD_P + 1) // 4, FIELD_P)
    if sig[32] > 1 or (y * y - x * x * x - 7) % FIELD_P:
        return EXCESS_BAD_R
    if (y > FIELD_P - y) != bool(sig[32]):
        y = FIELD_P - y
    X = excess_key_host(backend, setup, S, claim)
    if X is None:
        return EXCESS_NO_KEY
    c = excess_challenge(tag, sig[:33], X, msg)
    return 0 if _commit_terms(backend, [(s, B), (-c, X)]) == (x, y) else 1


# ---- the stated keys (bppp_rp_excess_keys / _verify_keys_* / _sums_*)
def excess_key33(X: Tuple[int, int]) -> bytes:
    """the 33 bytes of a key: put (x), then the sign byte (1 when y > p - y)"""
    return _point33(X)


def excess_lift33(b33: bytes) -> Optional[Tuple[int, int]]:
    """the point 33 bytes name, as the library lifts a key and the R of a signature: x reduced mod p, the root of x^3 + 7 with the stated sign; None
    when the sign byte is above 1 or x has no curve point"""
    x = decode_field(b33[:32], FIELD_P)
    y = pow((x * x * x + 7) % FIELD_P, (FIELD_P + 1) // 4, FIELD_P)
    if b33[32] > 1 or (y * y - x * x * x - 7) % FIELD_P:
        return None
    return (x, y if (y > FIELD_P - y) == bool(b33[32]) else FIELD_P - y)


def excess_verify_key_host(backend: "Backend", setup, key: bytes, msg: bytes, sig: bytes, tag: bytes = b"") -> int:
    """Host restatement of bppp_rp_excess_verify_keys_each for one (key, message, signature): the first verdict that applies, in the header's order.
    The challenge hashes the canonical bytes of the lifted key."""
    _, _, B = _excess_bases(setup)
    X = excess_lift33(key)
    if X is None:
        return EXCESS_BAD_KEY
    s = sum(int.from_bytes(sig[33 + 8 * i:41 + 8 * i], "big") << (64 * i) for i in range(4))
    if s >= N:
        return 3
    R = excess_lift33(sig[:33])
    if R is None:
        return EXCESS_BAD_R
    c = excess_challenge(tag, sig[:33], X, msg)
    return 0 if _commit_terms(backend, [(s, B), (-c, X)]) == R else 1


def excess_sums_host(backend: "Backend", setup, S: Point, claim, keys: Sequence[bytes], malformed: bool = False):
    """Host restatement of bppp_rp_excess_sums_each for one sum S (None: the identity; malformed: some referenced x has no curve point) with the
    revealed claim (a, ty, o) ((a, o) on a binary setup) and the stated keys of its group: (verdict, S less the keys — None for the identity, a
    malformed sum and one with a key that does not lift)"""
    g, H0, B = _excess_bases(setup)
    a, ty, o = claim if H0 is not None else (claim[0], 0, claim[-1])
    if malformed:
        return 2, None
    Xs = [excess_lift33(k) for k in keys]
    if None in Xs:
        return EXCESS_BAD_KEY, None
    rest = _commit_terms(backend, [(1, S)] + [(-1, X) for X in Xs])
    if not 0 <= ty < N or not 0 <= o < N:
        return 3, rest
    want = _commit_terms(backend, [(a, g), (o, B)] + ([(ty, H0)] if H0 is not None else []))
    return (0 if rest == want else 1), rest


# ---- half-aggregate excess signatures (bppp_rp_excess_halfagg / _halfagg_verify, bppp_rp_verify_block_agg); include/bppp.h states every message
def EXCESS_AGG_BYTES(n: int) -> int:
    """BPPP_RP_EXCESS_AGG_BYTES: n rows of 33 bytes and one scalar"""
    return 33 * n + 32


def _halfagg_domain(part: bytes, tag: bytes) -> bytes:
    return hashlib.sha256(b"bppp/excess/halfagg/" + part + b"/v1" + tag).digest()


def _s_of(b32: bytes) -> int:
    return sum(int.from_bytes(b32[8 * i:8 * i + 8], "big") << (64 * i) for i in range(4))


def excess_halfagg_leaf(tag: bytes, r33: bytes, key33: bytes, msg: bytes) -> bytes:
    """leaf = SHA-256 (Dl || the 33 bytes of R as they stand || the canonical 33 bytes of the key: put (x mod p), the sign byte || msg): 130 bytes"""
    return hashlib.sha256(_halfagg_domain(b"leaf", tag) + r33 + _put(decode_field(key33[:32], FIELD_P)) + key33[32:33] + msg).digest()


def excess_halfagg_root(tag: bytes, leaves: Sequence[bytes]) -> bytes:
    """the root over the leaves in job order: pairs hashed as SHA-256 (Dn || left || right), an odd last node moved up unchanged, until one is left"""
    dn, level = _halfagg_domain(b"node", tag), list(leaves)
    if not level:
        raise ValueError("a tree needs a leaf")
    while len(level) > 1:
        level = [hashlib.sha256(dn + level[j] + level[j + 1]).digest() if j + 1 < len(level) else level[j] for j in range(0, len(level), 2)]
    return level[0]


def excess_halfagg_coef(tag: bytes, root: bytes, n: int, i: int) -> int:
    """z_i = decode (SHA-256 (Dz || root || le64 (n) || le64 (i))) mod n, 1 for 0: 80 bytes"""
    return decode_field(hashlib.sha256(_halfagg_domain(b"coef", tag) + root + n.to_bytes(8, "little") + i.to_bytes(8, "little")).digest(), N) or 1


def _halfagg_coefs(tag: bytes, keys, msgs, rows) -> Tuple[bytes, List[int]]:
    root = excess_halfagg_root(tag, [excess_halfagg_leaf(tag, r, k, m) for r, k, m in zip(rows, keys, msgs)])
    return root, [excess_halfagg_coef(tag, root, len(keys), i) for i in range(len(keys))]


def excess_halfagg_status(key: bytes, sig: bytes) -> int:
    """the aggregator's verdict on one signature: BAD_KEY, NOT_CANONICAL (s >= n), BAD_R or OK; no equation"""
    return EXCESS_BAD_KEY if excess_lift33(key) is None else 3 if _s_of(sig[33:]) >= N else EXCESS_BAD_R if excess_lift33(sig[:33]) is None else 0


def excess_halfagg_host(tag: bytes, keys: Sequence[bytes], msgs: Sequence[bytes], sigs: Sequence[bytes]) -> bytes:
    """Host restatement of bppp_rp_excess_halfagg: the aggregate bytes (b"" for no key; all zero when excess_halfagg_status refuses a signature)"""
    n = len(keys)
    if not n:
        return b""
    if any(excess_halfagg_status(k, s) for k, s in zip(keys, sigs)):
        return bytes(EXCESS_AGG_BYTES(n))
    rows = [s[:33] for s in sigs]
    _, z = _halfagg_coefs(tag, keys, msgs, rows)
    return b"".join(rows) + _put(sum(zi * _s_of(s[33:]) for zi, s in zip(z, sigs)) % N)


def excess_halfagg_verify_host(backend: "Backend", setup, keys: Sequence[bytes], msgs: Sequence[bytes], agg: bytes, tag: bytes = b""):
    """Host restatement of bppp_rp_excess_halfagg_verify: (accept, statuses, the left side  s_agg B - sum z_i (c_i X_i + R_i)  over the open keys, None
    for the identity)"""
    _, _, B = _excess_bases(setup)
    n = len(keys)
    if not n:
        return True, [], None
    rows, s_agg = [agg[33 * i:33 * i + 33] for i in range(n)], _s_of(agg[33 * n:])
    _, z = _halfagg_coefs(tag, keys, msgs, rows)
    Xs, Rs = [excess_lift33(k) for k in keys], [excess_lift33(r) for r in rows]
    pre = [EXCESS_BAD_KEY if X is None else EXCESS_BAD_R if R is None else None for X, R in zip(Xs, Rs)]
    terms = [(s_agg if s_agg < N else 0, B)]
    for i in range(n):
        if pre[i] is None:
            terms += [(-z[i] * excess_challenge(tag, rows[i], Xs[i], msgs[i]), Xs[i]), (-z[i], Rs[i])]
    point = _commit_terms(backend, terms)
    open_verdict = 3 if s_agg >= N else 0 if point is None else 1
    accept = all(p is None for p in pre) and s_agg < N and point is None
    return accept, [open_verdict if p is None else p for p in pre], point


def block_agg_weight(seed: bytes, nkeys: int, root: bytes, s32: bytes) -> int:
    """rho_A of bppp_rp_verify_block_agg: decode (SHA-256 (seed_1 || le64 (nkeys) || root || the 32 bytes of s_agg)) mod n, 1 for 0: 104 bytes; seed:
    block_seeds (seed)[1]"""
    return decode_field(hashlib.sha256(seed + nkeys.to_bytes(8, "little") + root + s32).digest(), N) or 1


# ---- sealed outputs (bppp_rp_seal / bppp_rp_scan): a one-sided receive; include/bppp.h states every message
SEAL_OK, SEAL_NOT_CANONICAL, SEAL_ZERO = 0, 1, 2
SCAN_FOREIGN, SCAN_OWNED, SCAN_BAD_HINT, SCAN_TAG_ONLY = 0, 1, 2, 3


def SEAL_BYTES(nranges: int) -> int:
    """BPPP_RP_SEAL_BYTES: the hint R (33 bytes), the view tag, 64 memo bytes per range"""
    return 34 + 64 * nranges


def _seal_domain(part: bytes, tag: bytes) -> bytes:
    return hashlib.sha256(b"bppp/seal/" + part + b"/v1" + tag).digest()


def seal_shared(tag: bytes, P: Tuple[int, int], r33: bytes) -> bytes:
    """ss = SHA-256 (Ds || put (P.x) || sign (P) || the 33 bytes of R as stored): 98 bytes"""
    return hashlib.sha256(_seal_domain(b"shared", tag) + _point33(P) + r33).digest()


def seal_view_tag(tag: bytes, ss: bytes) -> int:
    return hashlib.sha256(_seal_domain(b"tag", tag) + ss).digest()[0]


def seal_blind(tag: bytes, ss: bytes, i: int) -> int:
    return decode_field(hashlib.sha256(_seal_domain(b"blind", tag) + ss + i.to_bytes(4, "little")).digest(), N)


def seal_pad(tag: bytes, ss: bytes, i: int) -> bytes:
    dm = _seal_domain(b"memo", tag)
    return b"".join(hashlib.sha256(dm + ss + i.to_bytes(4, "little") + bytes([h])).digest() for h in (0, 1))


def _xor(a: bytes, b: bytes) -> bytes:
    return bytes(x ^ y for x, y in zip(a, b))


def seal_host(backend: "Backend", setup, view_key: bytes, r: int, outputs: Sequence[Tuple[int, int]], tag: bytes = b""):
    """Host restatement of bppp_rp_seal for one row: outputs = one (amount, type) per range (the type of a binary setup is ignored).  Returns
    (status, the seal's bytes, the blindings); a refused row has zero bytes and zero blindings."""
    _, H0, B = _excess_bases(setup)
    nr = len(outputs)
    types = [ty if H0 is not None else 0 for _, ty in outputs]
    A = excess_lift33(view_key)
    status = EXCESS_BAD_KEY if A is None else SEAL_NOT_CANONICAL if not 0 <= r < N or any(not 0 <= t < N for t in types) else SEAL_ZERO if r == 0 else SEAL_OK
    if status != SEAL_OK:
        return status, bytes(SEAL_BYTES(nr)), [0] * nr
    r33 = _point33(backend.commit([r], [B]))
    ss = seal_shared(tag, backend.commit([r], [A]), r33)
    memos = [_xor(_put(v % N) + _put(t), seal_pad(tag, ss, i)) for i, ((v, _), t) in enumerate(zip(outputs, types))]
    return status, r33 + bytes([seal_view_tag(tag, ss)]) + b"".join(memos), [seal_blind(tag, ss, i) for i in range(nr)]


def _seal_decode_com(coms_file: bytes, nr: int, i: int) -> Optional[Tuple[int, int]]:
    """commitment i of a commitments file (decodeCommitments, one point): None when its x has no curve point"""
    ns = (nr + 7) // 8
    return excess_lift33(coms_file[ns + 32 * i:ns + 32 * i + 32] + bytes([(coms_file[i >> 3] >> (i & 7)) & 1]))


def scan_host(backend: "Backend", setup, a: int, coms_file: bytes, seal: bytes, tag: bytes = b""):
    """Host restatement of bppp_rp_scan for one row under the view secret a (1 <= a < n): (verdict, [(amount, type, blinding)] per range); every
    row that is not owned has zeros."""
    g, H0, B = _excess_bases(setup)
    nr = (len(seal) - 34) // 64
    zeros = [(0, 0, 0)] * nr
    R = excess_lift33(seal[:33])
    if R is None:
        return SCAN_BAD_HINT, zeros
    ss = seal_shared(tag, backend.commit([a], [R]), seal[:33])
    if seal_view_tag(tag, ss) != seal[33]:
        return SCAN_FOREIGN, zeros
    out = []
    for i in range(nr):
        m = _xor(seal[34 + 64 * i:98 + 64 * i], seal_pad(tag, ss, i))
        v, ty, bl = _get256(m[:32]), _get256(m[32:]), seal_blind(tag, ss, i)
        C = _seal_decode_com(coms_file, nr, i)
        if v >= N or ty >= N or (H0 is None and ty) or C is None:          # a binary setup has no type base: a seal that carries a type names no commitment of it
            return SCAN_TAG_ONLY, zeros
        if C != _commit_terms(backend, [(v, g), (bl, B)] + ([(ty, H0)] if H0 is not None else [])):
            return SCAN_TAG_ONLY, zeros
        out.append((v, ty, bl))
    return SCAN_OWNED, out


SCAN_MAX_KEYS = 1 << 20


def scan_keys_host(backend: "Backend", setup, secrets: Sequence[int], files: Sequence[bytes], seals: Sequence[bytes], tag: bytes = b""):
    """Host restatement of bppp_rp_scan_keys: the literal K x rows loop over scan_host.  Returns (row_status, hits, ntag_only) — hits as (key, row,
    opening) ordered by (row, key); a row is BAD_HINT, else OWNED if some key owns it, else TAG_ONLY if some key's tag matched, else FOREIGN."""
    row_status, hits, ntag = [], [], 0
    for i, (f, s) in enumerate(zip(files, seals)):
        verdicts = []
        for k, a in enumerate(secrets):
            verdict, opening = scan_host(backend, setup, a, f, s, tag)
            verdicts.append(verdict)
            if verdict == SCAN_OWNED:
                hits.append((k, i, opening))
            ntag += verdict == SCAN_TAG_ONLY
        row_status.append(next((v for v in (SCAN_BAD_HINT, SCAN_OWNED, SCAN_TAG_ONLY) if v in verdicts), SCAN_FOREIGN))
    return row_status, hits, ntag


# ---- the multi-party signer (bppp_rp_excess_part_*): builders who each know a part e_i of the blinding sum; include/bppp.h states every message
EXCESS_PUBNONCE_BYTES = 66
EXCESS_PARTIAL_BYTES = 32
EXCESS_NONCE_INFINITY = 7
EXCESS_NO_AGGREGATE = 8


def _get256(b32: bytes) -> int:
    """the 256-bit integer 32 bytes hold as put wrote them, not reduced"""
    return sum(int.from_bytes(b32[8 * i:8 * i + 8], "big") << (64 * i) for i in range(4))


def excess_part_nonce(tag: bytes, e: int, msg: bytes, aux: bytes, j: int) -> int:
    """k_j = decode (SHA-256 (Dm || put (e) || msg || aux || byte j)) mod n for j = 1, 2, Dm = SHA-256 ("bppp/excess/partnonce/v1" || tag): 129 bytes"""
    return decode_field(hashlib.sha256(hashlib.sha256(b"bppp/excess/partnonce/v1" + tag).digest() + _put(e) + msg + aux + bytes([j])).digest(), N)


def excess_nonce_coef(tag: bytes, r1_33: bytes, r2_33: bytes, X: Tuple[int, int], msg: bytes) -> int:
    """b = decode (SHA-256 (Db || the canonical 33 bytes of R1agg || of R2agg || of X || msg)) mod n, Db = SHA-256 ("bppp/excess/noncecoef/v1" || tag):
    163 bytes"""
    return decode_field(hashlib.sha256(hashlib.sha256(b"bppp/excess/noncecoef/v1" + tag).digest() + r1_33 + r2_33 + _point33(X) + msg).digest(), N)


def _excess_part_status(e: int, tag: bytes, msg: bytes, aux: bytes):
    """the signer's verdict on its blinding part and the two nonces (None where refused)"""
    if not 0 <= e < N:
        return EXCESS_NOT_CANONICAL, None
    if e == 0:
        return EXCESS_ZERO, None
    ks = [excess_part_nonce(tag, e, msg, aux, j) for j in (1, 2)]
    return (EXCESS_NONCE, None) if 0 in ks else (EXCESS_OK, ks)


def excess_part_nonces_host(backend: "Backend", setup, e: int, msg: bytes, aux: bytes, tag: bytes = b""):
    """Host restatement of bppp_rp_excess_part_nonces for one session: (status, the 66 bytes of (k_1 B, k_2 B)); a refused row has zero bytes"""
    _, _, B = _excess_bases(setup)
    status, ks = _excess_part_status(e, tag, msg, aux)
    if status != EXCESS_OK:
        return status, bytes(EXCESS_PUBNONCE_BYTES)
    return status, b"".join(_point33(backend.commit([k], [B])) for k in ks)


def _excess_part_group(backend: "Backend", pubnonces: Sequence[bytes], keys: Sequence[bytes]):
    """the stage of bppp_rp_excess_part_aggregate for one sum: (verdict, R1agg, R2agg, X), the points None unless the verdict is OK"""
    Xs = [excess_lift33(k) for k in keys]
    if None in Xs:
        return EXCESS_BAD_KEY, None, None, None
    R1s, R2s = [excess_lift33(pn[:33]) for pn in pubnonces], [excess_lift33(pn[33:]) for pn in pubnonces]
    if None in R1s or None in R2s:
        return EXCESS_BAD_R, None, None, None
    X, R1, R2 = (_commit_terms(backend, [(1, p) for p in ps]) for ps in (Xs, R1s, R2s))
    if X is None:
        return EXCESS_NO_KEY, None, None, None
    if R1 is None or R2 is None:
        return EXCESS_NONCE_INFINITY, None, None, None
    return EXCESS_OK, R1, R2, X


def _excess_part_session(backend: "Backend", tag: bytes, R1, R2, X, msg: bytes):
    """(b, R, c) of a session; R None (and c None) when R1agg + b R2agg is infinity"""
    b = excess_nonce_coef(tag, _point33(R1), _point33(R2), X, msg)
    R = _commit_terms(backend, [(1, R1), (b, R2)])
    return b, R, (excess_challenge(tag, _point33(R), X, msg) if R is not None else None)


def excess_part_aggregate_host(backend: "Backend", setup, pubnonces: Sequence[bytes], keys: Sequence[bytes]):
    """Host restatement of bppp_rp_excess_part_aggregate for one sum: (status, the 66 bytes of (R1agg, R2agg), the 33 bytes of X); zero bytes when refused"""
    status, R1, R2, X = _excess_part_group(backend, pubnonces, keys)
    if status != EXCESS_OK:
        return status, bytes(EXCESS_PUBNONCE_BYTES), bytes(EXCESS_KEY_BYTES)
    return status, _point33(R1) + _point33(R2), _point33(X)


def excess_part_sign_host(backend: "Backend", setup, e: int, msg: bytes, aux: bytes, agg_nonce: bytes, agg_key: bytes, tag: bytes = b""):
    """Host restatement of bppp_rp_excess_part_sign for one session: (status, put (k_1 + b k_2 + c e)); zero bytes when refused"""
    refused = lambda st: (st, bytes(EXCESS_PARTIAL_BYTES))
    status, ks = _excess_part_status(e, tag, msg, aux)
    if status != EXCESS_OK:
        return refused(status)
    X, R1, R2 = excess_lift33(agg_key), excess_lift33(agg_nonce[:33]), excess_lift33(agg_nonce[33:])
    if X is None:
        return refused(EXCESS_BAD_KEY)
    if R1 is None or R2 is None:
        return refused(EXCESS_BAD_R)
    b, R, c = _excess_part_session(backend, tag, R1, R2, X, msg)
    if R is None:
        return refused(EXCESS_NONCE_INFINITY)
    return EXCESS_OK, _put((ks[0] + b * ks[1] + c * e) % N)


def excess_part_verify_host(backend: "Backend", setup, pubnonces: Sequence[bytes], keys: Sequence[bytes], partials: Sequence[bytes], msg: bytes, tag: bytes = b""):
    """Host restatement of bppp_rp_excess_part_verify for one sum: (the verdict of every part, the verdict of the sum), in the header's order"""
    _, _, B = _excess_bases(setup)
    sum_status, R1, R2, X = _excess_part_group(backend, pubnonces, keys)
    b = c = None
    if sum_status == EXCESS_OK:
        b, R, c = _excess_part_session(backend, tag, R1, R2, X, msg)
        if R is None:
            sum_status = EXCESS_NONCE_INFINITY
    out = []
    for pn, key, part in zip(pubnonces, keys, partials):
        Xi, R1i, R2i, s = excess_lift33(key), excess_lift33(pn[:33]), excess_lift33(pn[33:]), _get256(part)
        if Xi is None:
            out.append(EXCESS_BAD_KEY)
        elif s >= N:
            out.append(3)
        elif R1i is None or R2i is None:
            out.append(EXCESS_BAD_R)
        elif sum_status in (EXCESS_BAD_KEY, EXCESS_BAD_R):
            out.append(EXCESS_NO_AGGREGATE)                 # another part of the sum does not lift
        elif sum_status != EXCESS_OK:
            out.append(sum_status)
        else:
            out.append(0 if _commit_terms(backend, [(s, B), (-b, R2i), (-c, Xi)]) == R1i else 1)
    return out, sum_status


def excess_part_combine_host(backend: "Backend", setup, pubnonces: Sequence[bytes], keys: Sequence[bytes], partials: Sequence[bytes], msg: bytes, tag: bytes = b""):
    """Host restatement of bppp_rp_excess_part_combine for one sum: (status, the 65 signature bytes, the 33 bytes of the aggregated key); zero bytes when
    refused.  The partials are added mod n as they are: nothing checks them here."""
    status, R1, R2, X = _excess_part_group(backend, pubnonces, keys)
    R = None
    if status == EXCESS_OK:
        _, R, _ = _excess_part_session(backend, tag, R1, R2, X, msg)
        if R is None:
            status = EXCESS_NONCE_INFINITY
    if status != EXCESS_OK:
        return status, bytes(EXCESS_SIG_BYTES), bytes(EXCESS_KEY_BYTES)
    return status, _point33(R) + _put(sum(_get256(p) for p in partials) % N), _point33(X)


def _mixed_groups(files):
    """bppp_rp_group[] for (handle, batch, coms pointer, proofs pointer) rows; every handle on one context"""
    from .capi import RpGroup
    arr = (RpGroup * max(len(files), 1))()
    for g, (nat, B, pc, pp) in zip(arr, files):
        g.rp, g.batch, g.coms_files, g.proof_files = (nat.h.value if nat.h else None), B, pc, pp
    return arr


def verify_mixed(gpu, groups, seed: Optional[bytes] = None, want_status: bool = False):
    """bppp_rp_verify_mixed: proofs of SEVERAL setups in one call and one combined MSM.  groups = [(NativeRangeProofs or
    NativeBinaryRangeProofs, commitments files, proof files)]; the job is the groups concatenated in order.  Returns accept, or
    (accept, status list in job order) with want_status.  A file of the wrong length makes the whole job MALFORMED without a library
    call, as NativeRangeProofs.verify_batch does for its batch.  `seed`: fresh from os.urandom unless given (fixed seeds are for tests)."""
    import ctypes as C
    import numpy as np
    if seed is None:
        seed = os.urandom(32)
    if len(seed) != 32:
        raise ValueError("a 32-byte seed is required")
    groups = [(nat, list(cf), list(pf)) for nat, cf, pf in groups]
    if any(len(cf) != len(pf) for _, cf, pf in groups):
        raise ValueError("one commitments file per proof is required")
    total = sum(len(pf) for _, _, pf in groups)
    if any(len(c) != nat.shape["coms_bytes"] for nat, cf, _ in groups for c in cf) or \
            any(len(p_) != nat.shape["proof_bytes"] for nat, _, pf in groups for p_ in pf):
        return (False, [2] * total) if want_status else False
    keep = [(np.frombuffer(b"".join(cf) or b"\0", dtype=np.uint8), np.frombuffer(b"".join(pf) or b"\0", dtype=np.uint8)) for _, cf, pf in groups]
    arr = _mixed_groups([(nat, len(pf), cb.ctypes.data, pb.ctypes.data) for (nat, _, pf), (cb, pb) in zip(groups, keep)])
    acc = C.c_int(0)
    status = np.zeros(max(total, 1), dtype=np.uint32)
    sd = np.frombuffer(seed, dtype=np.uint8)
    rc = gpu.lib.bppp_rp_verify_mixed(C.cast(arr, C.c_void_p), len(groups), C.c_void_p(sd.ctypes.data), C.byref(acc),
                                      C.c_void_p(status.ctypes.data) if want_status else None, None)
    gpu._check(rc, "bppp_rp_verify_mixed")
    return (bool(acc.value), [int(v) for v in status[:total]]) if want_status else bool(acc.value)


def prove_mixed(gpu, groups):
    """bppp_rp_prove_mixed: a job of SEVERAL setups in one call.  groups = [(NativeRangeProofs or NativeBinaryRangeProofs, inputs,
    rand_prefixes)] or, with per-proof public amounts, [(handle, inputs, rand_prefixes, public_amounts)] — each as that handle's
    prove_batch takes them.  Returns one list of (commitments file, proof file) per group, the bytes prove_batch gives.  Handles whose
    bases extend one another prove over one shared comb table afterwards (see NativeRangeProofs.share_comb)."""
    import ctypes as C
    from .capi import RpProveGroup
    groups = [tuple(g) + (None,) * (4 - len(g)) for g in groups]
    arr = (RpProveGroup * max(len(groups), 1))()
    keep, outs = [], []
    vp = lambda a: a.ctypes.data
    for g, (nat, inputs, prefixes, pub) in zip(arr, groups):
        B = len(inputs)
        g.rp, g.batch = (nat.h.value if nat.h else None), B
        if B == 0:
            outs.append(None)
            continue
        amt, typ, bld, pre, plen, cf, pf = nat._prove_arrays(nat._prove_rows(inputs), prefixes)
        words = None if pub is None else nat._public_words(pub, B)
        keep.append((amt, typ, bld, pre, cf, pf, words))
        g.amounts, g.types, g.blinds, g.rand_prefix, g.prefix_len, g.coms_files, g.proof_files = vp(amt), vp(typ), vp(bld), vp(pre), plen, vp(cf), vp(pf)
        g.public_amounts = None if words is None else vp(words)
        outs.append((cf, pf))
    gpu._check(gpu.lib.bppp_rp_prove_mixed(C.cast(arr, C.c_void_p), len(groups)), "bppp_rp_prove_mixed")
    return [[] if o is None else nat._prove_files(len(inputs), *o) for o, (nat, inputs, _, _) in zip(outs, groups)]


def verify_mixed_device(gpu, groups, seed: bytes, index_offset: int = 0):
    """bppp_rp_verify_mixed_device: groups = [(handle, batch, device pointer of the commitments files, of the proof files)], the job's
    proofs at positions [index_offset, index_offset + total batch) (a rank's share of a sharded mixed job).  Returns (accept, status list
    in job order, the combined point) — the combined point is the sum of every group's verify_batch_device_point at its offset."""
    import ctypes as C
    import numpy as np
    from .capi import array_to_point
    groups = list(groups)
    total = sum(B for _, B, _, _ in groups)
    arr = _mixed_groups([(nat, B, int(pc), int(pp)) for nat, B, pc, pp in groups])
    acc, out = C.c_int(0), np.zeros(8, dtype=np.uint64)
    status = np.zeros(max(total, 1), dtype=np.uint32)
    sd = np.frombuffer(seed, dtype=np.uint8)
    rc = gpu.lib.bppp_rp_verify_mixed_device(C.cast(arr, C.c_void_p), len(groups), index_offset, C.c_void_p(sd.ctypes.data), C.byref(acc),
                                             C.c_void_p(status.ctypes.data), C.c_void_p(out.ctypes.data))
    gpu._check(rc, "bppp_rp_verify_mixed_device")
    return bool(acc.value), [int(v) for v in status[:total]], array_to_point(out)


# ----------------------------------------------------------------------------- schema files (app/Parse.hs, app/Main.hs)
def approx_log_w(n: int) -> int:
    """approxLogW (app/Parse.hs:202-206): the default base for a range of width n"""
    l = integer_log(2, n)
    return l // integer_log(2, l)


def setup_from_schema(backend: Backend, schema: dict, points: Optional[Sequence[Point]] = None) -> SetupTRRP:
    """The reciprocal branch of the CLI's schema handling (app/Parse.hs:100-186, app/Main.hs:262-285): defaults argument = IP,
    count = 1, min = 0, max = 2^64, base = approxLogW (max - min), flags False; typed or conserved => hasTypes.  `points`
    defaults to the try-and-increment stream over schema["basisSeed"] (getPoints, app/Main.hs:68-72; even-y root: this build's
    documented choice).  Binary schemas ("binary": true) are a different protocol (RangeProof.Binary): they go through
    bulletproofspp_amd.rangeproof_binary.setup_from_schema and are refused here."""
    if schema.get("binary", False):
        raise ValueError("a binary schema (RangeProof.Binary): use bulletproofspp_amd.rangeproof_binary.setup_from_schema")
    arg = str(schema.get("argument", "IP")).lower()
    flavour = {"ip": "IP", "innerproduct": "IP", "nl": "NL", "normlinear": "NL"}.get(arg)
    if flavour is None:
        raise ValueError("Unsupported Argument: " + arg)
    has_types = bool(schema.get("typed", False)) or bool(schema.get("conserved", False))
    rds: List[RangeData] = []
    for r in schema["ranges"]:
        lo, hi = int(r.get("min", 0)), int(r.get("max", 2**64))
        base = int(r["base"]) if "base" in r else approx_log_w(hi - lo)
        rd = make_range_data(base, lo, hi, bool(r.get("isShared", False)), bool(r.get("isOutput", False)), bool(r.get("isAssumed", False)))
        if rd is None:
            raise ValueError("Invalid range: %r" % (r,))
        rds += [rd] * int(r.get("count", 1))
    pubs = []
    for pb in schema.get("public", []):
        if pb.get("blind") is not None:
            raise ValueError("Cannot have blinding on public value")
        pubs.append((bool(pb.get("isOutput", False)), int(pb.get("type", 0)), int(pb["amount"])))
    if points is None:
        if "basisSeed" not in schema:
            raise ValueError("no basis: pass points or give basisSeed")
        nrm_len = sum(len(rd.base_coeffs) + (1 if has_types else 0) for rd in rds)
        points = basis_points(str(schema["basisSeed"]).encode(), 2 + nrm_len + 6 + sum(rd.base for rd in rds if rd.is_shared) + 2)
    return setup(backend, points, has_types, pubs, rds, flavour)


def inputs_from_witness(witness_json: Sequence[dict], random_seed: bytes = b"default random seed") -> List[Tuple[int, int, int]]:
    """(amount, type, blinding) per entry; missing blindings come from hashToScalars ("Blinding " <> seed) numbered from 1
    (app/Main.hs:86-87, :252-253)"""
    gen = hash_to_scalar(b"Blinding " + random_seed)
    return [(int(w["amount"]), int(w.get("type", 0)), int(w["blind"]) if w.get("blind") is not None else gen(i + 1)) for i, w in enumerate(witness_json)]


def basis_points(seed: bytes, count: int) -> List[Point]:
    """getPoints (app/Main.hs:68-72): x = hash (seed <> show n) for n = 0, 1, ... — the digest decoded by Binary (Prime p)
    (decode_field, Encoding.hs:75-79) — kept when x^3 + 7 is a square (pointX); the root taken is the even one (the
    reference's `sr` choice cannot be confirmed offline)."""
    p = 2**256 - 2**32 - 977
    out, n = [], 0
    while len(out) < count:
        x = decode_field(hashlib.sha256(seed + str(n).encode()).digest(), p)
        n += 1
        rhs = (x * x * x + 7) % p
        y = pow(rhs, (p + 1) // 4, p)
        if y * y % p != rhs:
            continue
        out.append((x, p - y if y & 1 else y))
    return out


# ---- set commitments (bppp_rp_set_*): an append-only Merkle mountain range over opaque rows; include/bppp.h states every message.  The functions
# below restate it with hashlib, and CommitmentSet wraps the device-resident set
SET_OK, SET_MISMATCH, SET_BAD_INDEX, SET_BAD_PADDING = 0, 1, 2, 3
SET_MAX_ROW_BYTES = 8192


def _set_domain(part: bytes, tag: bytes) -> bytes:
    return hashlib.sha256(b"bppp/set/" + part + b"/v1" + tag).digest()


def set_path_bytes(n: int) -> int:
    """bppp_rp_set_path_bytes: 32 bit_length (n)"""
    return 32 * int(n).bit_length()


def set_leaf_host(tag: bytes, row: bytes) -> bytes:
    """leaf = SHA-256 (Dl || row)"""
    return hashlib.sha256(_set_domain(b"leaf", tag) + row).digest()


def _set_peak_levels(n: int) -> List[int]:
    """the levels of P_0 .. P_{m-1}: the set bits of n from the highest down"""
    return [k for k in range(n.bit_length() - 1, -1, -1) if (n >> k) & 1]


def set_peaks_host(tag: bytes, rows: Sequence[bytes], start: Optional[Tuple[int, Sequence[bytes]]] = None) -> List[bytes]:
    """The peaks P_0 .. P_{m-1} after `rows` were appended to an empty set, or to the state start = (n, its peaks): a stack of (level, node) whose two
    topmost nodes merge into SHA-256 (Dn || left || right) whenever their levels are equal"""
    dl, dn = _set_domain(b"leaf", tag), _set_domain(b"node", tag)
    n0, peaks0 = start if start is not None else (0, [])
    stack = list(zip(_set_peak_levels(n0), peaks0))
    if len(stack) != bin(n0).count("1"):
        raise ValueError("a state of n rows has popcount (n) peaks")
    for row in rows:
        stack.append((0, hashlib.sha256(dl + row).digest()))
        while len(stack) > 1 and stack[-1][0] == stack[-2][0]:
            (k, right), (_, left) = stack.pop(), stack.pop()
            stack.append((k + 1, hashlib.sha256(dn + left + right).digest()))
    return [h for _, h in stack]


def _set_bag(tag: bytes, peaks: Sequence[bytes]) -> bytes:
    if not peaks:
        return bytes(32)
    db, acc = _set_domain(b"bag", tag), peaks[-1]
    for p in reversed(peaks[:-1]):
        acc = hashlib.sha256(db + p + acc).digest()
    return acc


def set_root_host(tag: bytes, row_bytes: int, n: int, peaks: Sequence[bytes]) -> bytes:
    """root = SHA-256 (Dr || le64 (n) || le32 (row_bytes) || bag), bag = P_{m-1} folded leftwards by SHA-256 (Db || P_i || acc); zeros for n = 0"""
    return hashlib.sha256(_set_domain(b"root", tag) + n.to_bytes(8, "little") + row_bytes.to_bytes(4, "little") + _set_bag(tag, peaks)).digest()


def set_levels_host(tag: bytes, rows: Sequence[bytes]) -> List[List[bytes]]:
    """every node of the set of `rows`: levels[k][j] = node (k, j) for j < n >> k"""
    dn = _set_domain(b"node", tag)
    levels = [[set_leaf_host(tag, r) for r in rows]]
    while len(levels[-1]) > 1:
        lo = levels[-1]
        levels.append([hashlib.sha256(dn + lo[2 * j] + lo[2 * j + 1]).digest() for j in range(len(lo) // 2)])
    return levels


def _set_locate(n: int, i: int) -> Tuple[int, int, int]:
    """(h, p, m) of leaf i < n: its peak P_p of height h among the m peaks"""
    start = 0
    for p, k in enumerate(_set_peak_levels(n)):
        if i < start + (1 << k):
            return k, p, bin(n).count("1")
        start += 1 << k
    raise ValueError("i is not below n")


def set_path_host(tag: bytes, rows: Sequence[bytes], i: int, levels: Optional[List[List[bytes]]] = None) -> bytes:
    """The path of leaf i among the rows: the h siblings inside its peak bottom-up, the bag of the peaks to the right as one hash (if any), the peaks
    to the left nearest first, zero bytes up to 32 bit_length (n).  levels: set_levels_host (tag, rows), to share among calls"""
    n = len(rows)
    levels = levels if levels is not None else set_levels_host(tag, rows)
    h, p, m = _set_locate(n, i)
    peaks = [levels[k][(n >> k) - 1] for k in _set_peak_levels(n)]
    out = [levels[s][(i >> s) ^ 1] for s in range(h)]
    if p < m - 1:
        out.append(_set_bag(tag, peaks[p + 1:]))
    out += peaks[:p][::-1]
    assert len(out) <= n.bit_length()
    return b"".join(out).ljust(set_path_bytes(n), b"\0")


def set_verify_path_host(tag: bytes, row_bytes: int, n: int, root: bytes, i: int, row: bytes, path: bytes) -> int:
    """Host restatement of one query of bppp_rp_set_verify_paths; the first verdict that applies: SET_BAD_INDEX, SET_BAD_PADDING, SET_MISMATCH, SET_OK"""
    if len(row) != row_bytes or len(path) != set_path_bytes(n):
        raise ValueError("a row has row_bytes bytes and a path 32 bit_length (n)")
    if not 0 <= i < n:
        return SET_BAD_INDEX
    h, p, m = _set_locate(n, i)
    used = h + (1 if p < m - 1 else 0) + p
    if any(path[32 * used:]):
        return SET_BAD_PADDING
    dn, db = _set_domain(b"node", tag), _set_domain(b"bag", tag)
    acc, hs = set_leaf_host(tag, row), [path[32 * s:32 * s + 32] for s in range(used)]
    for s in range(h):
        acc = hashlib.sha256(dn + hs[s] + acc).digest() if (i >> s) & 1 else hashlib.sha256(dn + acc + hs[s]).digest()
    if p < m - 1:
        acc = hashlib.sha256(db + acc + hs[h]).digest()
    for left in hs[used - p:]:
        acc = hashlib.sha256(db + left + acc).digest()
    got = hashlib.sha256(_set_domain(b"root", tag) + n.to_bytes(8, "little") + row_bytes.to_bytes(4, "little") + acc).digest()
    return SET_OK if got == root else SET_MISMATCH


class CommitmentSet:
    """A device-resident set commitment on a range-proof handle (bppp_rp_set_create / _restore): append rows, read the root, the peaks and membership
    paths.  keep_nodes=False keeps the peaks alone and serves no paths.  Close it before its handle."""

    def __init__(self, nat: "NativeRangeProofs", row_bytes: int, keep_nodes: bool = True, _handle=None):
        import ctypes as C
        self.nat, self.row_bytes, self.keep_nodes, self.h = nat, int(row_bytes), bool(keep_nodes), None
        if _handle is None:
            _handle = C.c_void_p()
            nat.gpu._check(nat.gpu.lib.bppp_rp_set_create(nat.h, self.row_bytes, 1 if keep_nodes else 0, C.byref(_handle)), "bppp_rp_set_create")
        self.h = _handle

    @classmethod
    def restore(cls, nat: "NativeRangeProofs", row_bytes: int, n: int, peaks: Sequence[bytes]) -> "CommitmentSet":
        """bppp_rp_set_restore: a frontier-only set of n rows that continues from the peaks another set exported"""
        import ctypes as C
        import numpy as np
        if len(peaks) != bin(n).count("1") or any(len(p) != 32 for p in peaks):
            raise ValueError("a state of n rows has popcount (n) peaks of 32 bytes")
        pk = np.frombuffer(b"".join(peaks) or b"\0", dtype=np.uint8)
        hnd = C.c_void_p()
        nat.gpu._check(nat.gpu.lib.bppp_rp_set_restore(nat.h, int(row_bytes), int(n), C.c_void_p(pk.ctypes.data), C.byref(hnd)), "bppp_rp_set_restore")
        return cls(nat, row_bytes, False, _handle=hnd)

    def _live(self):
        if not self.h or not self.nat.h:
            raise ValueError("the set or its handle is closed")
        return self.nat.gpu

    def close(self):
        if self.h:
            self.nat.gpu.lib.bppp_rp_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append(self, rows) -> None:
        """bppp_rp_set_append: rows as a sequence of row_bytes-long byte strings, or as their concatenation"""
        import ctypes as C
        import numpy as np
        g = self._live()
        blob = bytes(rows) if isinstance(rows, (bytes, bytearray, memoryview)) else b"".join(rows)
        if len(blob) % self.row_bytes or (not isinstance(rows, (bytes, bytearray, memoryview)) and any(len(r) != self.row_bytes for r in rows)):
            raise ValueError("every row has row_bytes bytes")
        arr = np.frombuffer(blob or b"\0", dtype=np.uint8)
        g._check(g.lib.bppp_rp_set_append(self.h, len(blob) // self.row_bytes, C.c_void_p(arr.ctypes.data)), "bppp_rp_set_append")

    def info(self) -> dict:
        """bppp_rp_set_info: n, row_bytes, npeaks, store_bytes"""
        import ctypes as C
        g = self._live()
        n, rb, npk, sb = C.c_uint64(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        g._check(g.lib.bppp_rp_set_info(self.h, C.byref(n), C.byref(rb), C.byref(npk), C.byref(sb)), "bppp_rp_set_info")
        return {"n": int(n.value), "row_bytes": int(rb.value), "npeaks": int(npk.value), "store_bytes": int(sb.value)}

    def root(self) -> bytes:
        """bppp_rp_set_root"""
        import ctypes as C
        g = self._live()
        buf = (C.c_uint8 * 32)()
        g._check(g.lib.bppp_rp_set_root(self.h, C.cast(buf, C.c_void_p)), "bppp_rp_set_root")
        return bytes(buf)

    def peaks(self) -> List[bytes]:
        """bppp_rp_set_peaks: P_0 .. P_{m-1}"""
        import ctypes as C
        g = self._live()
        m = self.info()["npeaks"]
        buf = (C.c_uint8 * max(32 * m, 1))()
        g._check(g.lib.bppp_rp_set_peaks(self.h, C.cast(buf, C.c_void_p)), "bppp_rp_set_peaks")
        out = bytes(buf)
        return [out[32 * p:32 * p + 32] for p in range(m)]

    def paths(self, idx: Sequence[int]) -> List[bytes]:
        """bppp_rp_set_paths: the paths of the leaves idx against the rows there are now"""
        import ctypes as C
        import numpy as np
        g = self._live()
        pb, nq = set_path_bytes(self.info()["n"]), len(idx)
        ix = np.array(list(idx) or [0], dtype=np.uint64)
        buf = np.empty(max(nq * pb, 1), dtype=np.uint8)
        g._check(g.lib.bppp_rp_set_paths(self.h, nq, C.c_void_p(ix.ctypes.data), C.c_void_p(buf.ctypes.data)), "bppp_rp_set_paths")
        out = buf.tobytes()
        return [out[pb * q:pb * q + pb] for q in range(nq)]
