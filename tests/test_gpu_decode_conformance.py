"""The verifier's device decoders against the wire-format restatement: what a particular file MUST decode to, and which mutated files the
verifier must still accept.

The stage under test turns untrusted bytes into field elements and points: k_rp_decode_points / k_rp_decode_scalars (csrc/rpdecode.hip.h),
run alone through bppp_test_rp_decode_device — the launch the verifier makes — and the two other copies of the lift, k_lift_x
(bppp_lift_x_device) and seed_lift_digest.  Every expected value is computed here from bulletproofspp_amd/encoding.py (get_field, the sign
rule of decode_commitments) and the CPU oracle's lift_x; none comes from the library.

 a. crafted files (arbitrary bytes of the right length, positions filled from a corpus of edge values: 0, p - 1, the aliases p .. p + 40 and
    2^256 - 1 that only toP's conditional subtraction maps back, single-word and all-distinct-byte patterns that show a word or byte swap,
    both sign bits for every x, scalars at n - 1, n, n + 1, 2^256 - n) through four handles whose dimensions differ; exact points, scalars,
    bad[b] and any_bad; pad bits of the last sign byte ignored;
 b. bppp_lift_x_device and the seed stream's lift on the same corpus (the first REJECTS x >= p, the second reduces, like the file decoder);
 c. verdict parity: one honest proof per setup, every single-field mutation of it, verify_batch and verify_each under both hashing routes
    (host_oracle_max 0: device; a value that covers the batch, and slices of 8 under the defaults: host) against the host protocol verifier on
    the CPU oracle — accepting what it rejects is a soundness bug, rejecting what it accepts (set pad
    bits) a consensus split."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

from bulletproofspp_amd import encoding as E
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import array_to_point, array_to_scalars, load_test_library, scalars_to_array
from rp_backends import OracleBackend
from test_rangeproof import EXAMPLES

pytestmark = pytest.mark.gpu

P, N = E.P, RP.N
M64 = 2**64 - 1
DISTINCT = int.from_bytes(bytes(range(1, 33)), "big")            # 32 distinct bytes: any word or byte swap changes the value
# 64bit: inner-product flavour, ONE input commitment; rec_test: three; 32by64: norm-linear, 32 (four full sign bytes); bin_test: binary, two
# range-proof commitments.  Proof-file points: 10, 14, 18, 14 — none a multiple of 8.
SETUPS = ["64bit", "rec_test", "32by64", "bin_test"]
BIG = 45                                                          # proofs of the batch whose lanes cross wavefront and proof boundaries


# ----------------------------------------------------------------------------- the corpus (pure CPU)
def x_corpus():
    rnd = random.Random("decode conformance x")
    xs = [0, 1, 2, 3, 7, P - 2, P - 1] + [P + d for d in range(41)] + [2**256 - 1, 2**255] + [M64 << (64 * w) for w in range(4)] + [DISTINCT]
    return xs + [rnd.getrandbits(256) for _ in range(300)]


def scalar_corpus():
    rnd = random.Random("decode conformance scalars")
    ss = [0, 1, N - 1, N, N + 1, 2**256 - 1, 2**256 - N, 2**255] + [M64 << (64 * w) for w in range(4)] + [DISTINCT]
    return ss + [rnd.getrandbits(256) for _ in range(80)]


class Lift:
    """the oracle's root of x^3 + 7 for x < p (None: not on the curve), remembered"""

    def __init__(self, ec):
        self.ec, self.memo = ec, {}

    def __call__(self, x):
        assert 0 <= x < P
        if x not in self.memo:
            self.memo[x] = self.ec.lift_x(x)
        return self.memo[x]

    def many(self, xs):
        return [self(x) for x in xs]


def check_corpus(lift):
    """the conditions a corpus must meet before it is worth a GPU call"""
    xs = x_corpus()
    below = [x for x in xs if x < P]
    alias = [x for x in xs if x >= P]
    assert sum(lift(x) is not None for x in below) >= 8 and sum(lift(x) is None for x in below) >= 8
    assert sum(lift(x - P) is not None for x in alias) >= 3 and sum(lift(x - P) is None for x in alias) >= 3
    assert all(x < 2**256 for x in xs) and len(set(xs)) == len(xs)
    for r in below:
        pt = lift(r)
        assert pt is None or (pt[0] == r and (pt[1] * pt[1] - r * r * r - 7) % P == 0)
    return xs


@pytest.fixture(scope="module")
def lift(oracle_lib):
    lf = Lift(oracle_lib)
    check_corpus(lf)
    return lf


# ----------------------------------------------------------------------------- the wire format, restated per point
class Layout:
    """where the fields of the two files sit (encoding.py's docstring): proof file = scalars | sign bytes | x of rpComs ++ bpComs;
    commitments file = sign bytes | x of the inputs"""

    def __init__(self, shape, nrp):
        self.nrp, self.nr, self.k, self.fn, self.fl = nrp, shape["nranges"], shape["rounds"], shape["final_norm"], shape["final_lin"]
        self.ns, self.npp = self.fn + self.fl, nrp + 2 * shape["rounds"]
        self.p_signs, self.p_xs = 32 * self.ns, 32 * self.ns + (self.npp + 7) // 8
        self.c_signs, self.c_xs = 0, (self.nr + 7) // 8
        self.coms_bytes, self.proof_bytes = self.c_xs + 32 * self.nr, self.p_xs + 32 * self.npp
        assert (self.coms_bytes, self.proof_bytes) == (shape["coms_bytes"], shape["proof_bytes"])
        self.npts = self.npp + self.nr

    def build(self, scalars, pts):
        """files of one proof from ns raw 256-bit scalars and npts (raw x, sign bit): the proof file's points first, then the inputs"""
        assert len(scalars) == self.ns and len(pts) == self.npts
        pf, cf = bytearray(self.proof_bytes), bytearray(self.coms_bytes)
        for i, s in enumerate(scalars):
            pf[32 * i:32 * i + 32] = E.put_field(s)
        for i, (x, sg) in enumerate(pts[:self.npp]):
            pf[self.p_xs + 32 * i:self.p_xs + 32 * i + 32] = E.put_field(x)
            pf[self.p_signs + (i >> 3)] |= sg << (i & 7)
        for i, (x, sg) in enumerate(pts[self.npp:]):
            cf[self.c_xs + 32 * i:self.c_xs + 32 * i + 32] = E.put_field(x)
            cf[self.c_signs + (i >> 3)] |= sg << (i & 7)
        return bytes(cf), bytes(pf)

    def pad_masks(self):
        """the unused high bits of the last sign byte of (proof file, commitments file); 0 = the byte is full"""
        return tuple((0xFF << (n % 8)) & 0xFF if n % 8 else 0 for n in (self.npp, self.nr))

    def with_pads(self, cf, pf, on):
        mp, mc = self.pad_masks()
        cf, pf = bytearray(cf), bytearray(pf)
        lp, lc = self.p_xs - 1, self.c_xs - 1
        pf[lp] = (pf[lp] | mp) if on else (pf[lp] & ~mp & 0xFF)
        cf[lc] = (cf[lc] | mc) if on else (cf[lc] & ~mc & 0xFF)
        return bytes(cf), bytes(pf)


def expect_point(xb, want_big, lift):
    """get_field, the oracle's root, fromXWithSign — the three steps of decode_commitments for one point"""
    x = E.get_field(xb, P)
    r = lift(x)
    if r is None:
        return None
    y = r[1]
    if (y > P - y) != want_big:
        y = P - y
    return (x, y)


def expect_file(L, cf, pf, lift):
    """(init points, response points, norm scalars, linear scalars, bad) the decode stage must produce for one proof"""
    sc = [E.get_field(pf[32 * i:32 * i + 32], N) for i in range(L.ns)]
    bit = lambda data, off, i: bool((data[off + (i >> 3)] >> (i & 7)) & 1)
    pp = [expect_point(pf[L.p_xs + 32 * i:L.p_xs + 32 * i + 32], bit(pf, L.p_signs, i), lift) for i in range(L.npp)]
    cp = [expect_point(cf[L.c_xs + 32 * i:L.c_xs + 32 * i + 32], bit(cf, L.c_signs, i), lift) for i in range(L.nr)]
    return pp[:L.nrp] + cp, pp[L.nrp:], sc[:L.fn], sc[L.fn:], any(p is None for p in pp + cp)


def run_decode(gpu, tl, nat, L, files):
    B = len(files)
    init, resp = np.zeros((B, L.nrp + L.nr, 8), dtype=np.uint64), np.zeros((B, 2 * L.k, 8), dtype=np.uint64)
    wn, wl = np.zeros((B, L.fn, 4), dtype=np.uint64), np.zeros((B, L.fl, 4), dtype=np.uint64)
    bad, any_bad = np.full(B, 0xDEAD, dtype=np.uint32), np.full(1, 0xDEAD, dtype=np.uint32)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    gpu._check(tl.bppp_test_rp_decode_device(nat.h, B, b"".join(c for c, _ in files), b"".join(p for _, p in files), vp(init), vp(resp), vp(wn), vp(wl), vp(bad), vp(any_bad)),
               "bppp_test_rp_decode_device")
    return init, resp, wn, wl, bad, any_bad


def check_decode(gpu, tl, nat, L, files, lift, label):
    init, resp, wn, wl, bad, any_bad = run_decode(gpu, tl, nat, L, files)
    want_bad = []
    for b, (cf, pf) in enumerate(files):
        w_init, w_resp, w_n, w_l, w_bad = expect_file(L, cf, pf, lift)
        assert [array_to_point(r) for r in init[b]] == w_init, (label, b, "init")
        assert [array_to_point(r) for r in resp[b]] == w_resp, (label, b, "resp")
        assert array_to_scalars(wn[b]) == w_n and array_to_scalars(wl[b]) == w_l, (label, b, "scalars")
        want_bad.append(w_bad)
    assert [bool(v) for v in bad] == want_bad, (label, "bad")
    assert bool(any_bad[0]) == any(want_bad), (label, "any_bad")
    return want_bad, (init, resp, wn, wl, bad, any_bad)


def _handle(gpu, ec, name):
    schema = json.load(open(os.path.join(EXAMPLES, name, "schema.json")))
    binary = bool(schema.get("binary", False))
    st = (BRP if binary else RP).setup_from_schema(OracleBackend(ec), schema)
    nat = (BRP.NativeBinaryRangeProofs if binary else RP.NativeRangeProofs)(gpu, st)
    return st, nat, binary


@pytest.fixture(scope="module")
def handles(gpu, oracle_lib):
    hs = {name: _handle(gpu, oracle_lib, name) for name in SETUPS}
    yield hs
    for _, nat, _ in hs.values():
        nat.close()


def test_the_setups_cover_partial_sign_bytes(handles):
    shapes = {name: Layout(nat.shape, 2 if binary else 4) for name, (_, nat, binary) in handles.items()}
    assert any(L.npp % 8 for L in shapes.values()) and any(L.nr % 8 for L in shapes.values())
    assert {L.nrp for L in shapes.values()} == {2, 4}
    assert any(L.nr > 8 for L in shapes.values())                 # a sign-byte index above 0 in the commitments file
    for L in shapes.values():                                     # the large batch of test_crafted_files: no multiple of a wavefront, several of them
        for lanes in (BIG * L.npts, BIG * L.ns):
            assert lanes % 64 and lanes > 128


# ----------------------------------------------------------------------------- a. crafted files through the hook
@pytest.mark.parametrize("name", SETUPS)
def test_crafted_files(gpu, handles, lift, name):
    _, nat, binary = handles[name]
    tl = load_test_library()
    L = Layout(nat.shape, 2 if binary else 4)
    rnd = random.Random("crafted " + name)
    xs, ss = x_corpus(), scalar_corpus()
    liftable = [x for x in xs if lift(x % P) is not None]
    nonlift = [x for x in xs if lift(x % P) is None]
    sc_at = lambda j: [ss[(j * L.ns + i) % len(ss)] for i in range(L.ns)]

    # the sweep: every x of the corpus under both sign bits, in shuffled order so every position class meets every kind of value
    slots = [(x, sg) for x in xs for sg in (0, 1)]
    rnd.shuffle(slots)
    nfiles = max(-(-len(slots) // L.npts), -(-len(ss) // L.ns))
    sweep = [L.build(sc_at(j), [slots[(j * L.npts + i) % len(slots)] for i in range(L.npts)]) for j in range(nfiles)]
    # ... in which every position class holds both outcomes in some proof, and some proof is bad (CPU, before the launch)
    cls = {"response": [], "rp": [], "input": []}
    for cf, pf in sweep:
        w_init, w_resp, _, _, _ = expect_file(L, cf, pf, lift)
        cls["response"] += w_resp; cls["rp"] += w_init[:L.nrp]; cls["input"] += w_init[L.nrp:]
    for k_, pts in cls.items():
        assert any(p is None for p in pts) and any(p is not None for p in pts), k_
    check_decode(gpu, tl, nat, L, sweep, lift, "sweep")

    # pad bits: the same batch with the unused high bits of both last sign bytes all 0, then all 1 — identical output
    assert any(L.pad_masks())
    outs = [run_decode(gpu, tl, nat, L, [L.with_pads(cf, pf, on) for cf, pf in sweep]) for on in (False, True)]
    for a, b in zip(*outs):
        assert np.array_equal(a, b)

    # batch of 1, nothing bad: any_bad stays 0
    clean = lambda j: L.build(sc_at(j), [(rnd.choice(liftable), rnd.randrange(2)) for _ in range(L.npts)])
    want_bad, _ = check_decode(gpu, tl, nat, L, [clean(0)], lift, "one")
    assert want_bad == [False]
    # batch of 3: a bad response in the first, a bad input commitment in the last, the middle clean
    three = []
    for j, pos in enumerate((L.nrp + 2 * L.k - 1, None, L.npp + L.nr - 1)):
        pts = [(rnd.choice(liftable), rnd.randrange(2)) for _ in range(L.npts)]
        if pos is not None:
            pts[pos] = (rnd.choice(nonlift), rnd.randrange(2))
        three.append(L.build(sc_at(j + 1), pts))
    want_bad, _ = check_decode(gpu, tl, nat, L, three, lift, "three")
    assert want_bad == [True, False, True]
    # the large batch: one bad point (an alias of a non-liftable x, in the proof's last position) in one proof in the middle
    big = [clean(j) for j in range(BIG)]
    pts = [(rnd.choice(liftable), rnd.randrange(2)) for _ in range(L.npts)]
    pts[L.npts - 1] = (next(x for x in nonlift if x >= P), 1)
    big[BIG // 2] = L.build(sc_at(7), pts)
    want_bad, out0 = check_decode(gpu, tl, nat, L, big, lift, "big")
    assert want_bad == [j == BIG // 2 for j in range(BIG)]
    # ... and with every pad bit set: the clean proofs stay clean
    want_bad, out1 = check_decode(gpu, tl, nat, L, [L.with_pads(cf, pf, True) for cf, pf in big], lift, "big, pad bits set")
    assert want_bad == [j == BIG // 2 for j in range(BIG)]
    for a, b in zip(out0, out1):
        assert np.array_equal(a, b)


# ----------------------------------------------------------------------------- b. the two other copies of the lift
def test_lift_x_device_and_seed_lift(gpu, lift):
    rnd = random.Random("lift_x conformance")
    xs = x_corpus() + [rnd.getrandbits(256) for _ in range(3000)]
    n = len(xs)
    assert n % 64
    d_x, d_p = gpu.to_device(scalars_to_array(xs)), gpu.to_device(np.zeros((n, 8), dtype=np.uint64))
    try:
        gpu.lift_x(d_x, n, d_p)
        out = gpu.download(d_p, (n, 8))
    finally:
        gpu.free(d_x); gpu.free(d_p)
    seen = {"point": 0, "none": 0, "above": 0}
    for x, row in zip(xs, out):
        got = array_to_point(row)
        if x >= P:                                                # not a coordinate: refused, NOT reduced (include/bppp.h)
            assert got is None, hex(x)
            seen["above"] += 1
            continue
        r = lift(x)
        want = None if r is None else (x, r[1] if r[1] % 2 == 0 else P - r[1])
        assert got == want, hex(x)
        if got is not None:
            assert (got[1] * got[1] - got[0] ** 3 - 7) % P == 0 and got[1] < P
        seen["point" if got else "none"] += 1
    assert seen["above"] >= 42 and seen["point"] > 1000 and seen["none"] > 1000

    # seed_lift_digest on the corpus as digests: it reduces (a digest is any 256 bits), then the even root.  The 32 bytes are the value in
    # the WIRE layout (put_field: four big-endian 64-bit words, least significant word first), which is how the seed stream reads a digest
    # — not the value as one big-endian integer
    tl = load_test_library()
    cs = x_corpus()
    m = len(cs)
    assert m % 64
    x, ok, pts = np.zeros((m, 4), dtype=np.uint64), np.zeros(m, dtype=np.uint32), np.zeros((m, 8), dtype=np.uint64)
    gpu._check(tl.bppp_test_seed_lift_digests(gpu.h, b"".join(E.put_field(v) for v in cs), m, C.c_void_p(x.ctypes.data), C.c_void_p(ok.ctypes.data),
                                              C.c_void_p(pts.ctypes.data)), "lift_digests")
    for k_, v in enumerate(cs):
        r = lift(v % P)
        want = None if r is None else (v % P, r[1] if r[1] % 2 == 0 else P - r[1])
        assert array_to_scalars(x[k_]) == [v % P], hex(v)
        assert bool(ok[k_]) == (want is not None) and array_to_point(pts[k_]) == want, hex(v)


# ----------------------------------------------------------------------------- c. verdict parity on single-field mutations
CLASSES = ["response point", "rp commitment", "input commitment", "norm scalar", "linear scalar", "sign bit", "proof pad bits", "commitments pad bits"]
SAMPLE = {"32by64": 2}                                            # mutants kept per class on the setup whose host verification is slow


def mutants(L, cf, pf, lift):
    """[(class, commitments file, proof file)]: every single-field mutation of one proof"""
    out = []

    def other_x(xb):
        x = E.get_field(xb, P)
        return E.put_field(next(c for c in range(x + 1, x + 200) if lift(c % P) is not None) % P)

    def put(data, off, new):
        d = bytearray(data); d[off:off + len(new)] = new
        return bytes(d)

    def flip(data, off, i):
        d = bytearray(data); d[off + (i >> 3)] ^= 1 << (i & 7)
        return bytes(d)

    for i in range(L.npp):
        o = L.p_xs + 32 * i
        out.append(("rp commitment" if i < L.nrp else "response point", cf, put(pf, o, other_x(pf[o:o + 32]))))
        out.append(("sign bit", cf, flip(pf, L.p_signs, i)))
    for i in range(L.nr):
        o = L.c_xs + 32 * i
        out.append(("input commitment", put(cf, o, other_x(cf[o:o + 32])), pf))
        out.append(("sign bit", flip(cf, L.c_signs, i), pf))
    for i in range(L.ns):
        v = (E.get_field(pf[32 * i:32 * i + 32], N) + 1) % N
        out.append(("norm scalar" if i < L.fn else "linear scalar", cf, put(pf, 32 * i, E.put_field(v))))
    mp, mc = L.pad_masks()
    if mp:
        out.append(("proof pad bits", cf, L.with_pads(cf, pf, True)[1]))
    if mc:
        out.append(("commitments pad bits", L.with_pads(cf, pf, True)[0], pf))
    assert all((c, p) != (cf, pf) for _, c, p in out)
    return out


@pytest.mark.parametrize("name", SETUPS)
def test_verdict_parity_on_single_field_mutations(gpu, handles, lift, name):
    st, nat, binary = handles[name]
    nrp = 2 if binary else 4
    L = Layout(nat.shape, nrp)
    wit = json.load(open(os.path.join(EXAMPLES, name, "witness.json")))
    rows = RP.inputs_from_witness(wit, b"conformance")
    (cf, pf), = nat.prove_batch([[(v, bl) for v, _, bl in rows] if binary else rows], [b"conformance " + name.encode()])
    ms = mutants(L, cf, pf, lift)
    if name in SAMPLE:                                            # the first and the last few of every class
        keep = []
        for c in CLASSES:
            of_c = [m_ for m_ in ms if m_[0] == c]
            keep += of_c[:SAMPLE[name] - 1] + of_c[SAMPLE[name] - 1:][-1:]
        ms = keep
    present = {c for c, _, _ in ms}
    # every class, but for pad bits of a sign byte that is full (32 input commitments)
    assert present == set(CLASSES) - ({"commitments pad bits"} if L.nr % 8 == 0 else set()) - ({"proof pad bits"} if L.npp % 8 == 0 else set())
    if name != "32by64":
        assert present == set(CLASSES)
    files = [("honest", cf, pf)] + ms[:len(ms) // 2] + [("honest", cf, pf)] + ms[len(ms) // 2:] + [("honest", cf, pf)]

    verify_host = BRP.verify if binary else RP.verify
    memo = {}

    def host_accepts(c, p):
        if (c, p) not in memo:
            dc = E.decode_commitments(L.nr, c, lift.many)
            proof = None if dc is None else E.decode_proof(nrp, st.rounds, st.final_lens, dc[0], p, lift.many)
            memo[(c, p)] = proof is not None and bool(verify_host(st, proof, RP.sha256_oracle()))
        return memo[(c, p)]

    want = [host_accepts(c, p) for _, c, p in files]
    for (cls, _, _), w in zip(files, want):                       # the reference side: both directions are exercised
        assert w == (cls in ("honest", "proof pad bits", "commitments pad bits")), cls
    seed = bytes(range(32))
    coms, prfs = [c for _, c, _ in files], [p for _, _, p in files]
    # The hashing route: a batch hashes on the host cores iff it holds at most host_oracle_max proofs; 2^64 - 1 is not "unlimited" but
    # restores the default (8 proofs when verifying, include/bppp.h).  So: 0 = every batch on the device; a finite value that covers the
    # whole batch = the host route; and the defaults, under which the whole batch is too long for the host route and slices of 8 are not.
    default_max = 8
    assert len(files) > default_max
    whole = lambda: (nat.verify_batch(coms, prfs, seed, want_status=True), nat.verify_each(coms, prfs))
    got = {}
    try:
        for label, host_oracle_max in (("device", 0), ("host", len(files)), ("defaults", 2**64 - 1)):
            assert host_oracle_max == 0 or host_oracle_max >= len(files)
            nat.set_option("host_oracle_max", host_oracle_max)
            (ok, status, _), each = whole()
            assert ok == all(s_ == 0 for s_ in status), label
            got[label + ", batch"], got[label + ", each"] = status, each
        # still at the defaults: slices of at most 8 files take the host route
        sliced_b, sliced_e = [], []
        for lo in range(0, len(files), default_max):
            c_, p_ = coms[lo:lo + default_max], prfs[lo:lo + default_max]
            ok, status, _ = nat.verify_batch(c_, p_, seed, want_status=True)
            assert ok == all(s_ == 0 for s_ in status), lo
            sliced_b += status; sliced_e += nat.verify_each(c_, p_)
        got["defaults, batches of 8"], got["defaults, each of 8"] = sliced_b, sliced_e
    finally:
        nat.set_option("host_oracle_max", 2**64 - 1)              # the defaults again: the handle is shared
    for label, status in got.items():
        assert [s_ == 0 for s_ in status] == want, (label, [(cls, s_) for (cls, _, _), s_, w in zip(files, status, want) if (s_ == 0) != w])
        assert status == got["device, batch"], label
