"""bppp_rp_excess_sign*, bppp_rp_excess_verify_each*, bppp_rp_excess_verify_batch*: a tally checked without revealing the blinding sum.

The reference side is the host protocol code over the oracle backend (tests/rp_backends.py): rangeproof.excess_sign_host / excess_verify_host
restate the signature over the oracle's group law, rangeproof.tally_sums the sums, rangeproof.excess_weight the batch weight — never the
library under test.  The pools are test_gpu_commit_open's 65 rows per setup, computed once and shared; every job is a few dozen sums."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from rp_backends import OracleBackend
from test_gpu_commit_open import _case, _native, _no_point_x, _ref_points, _set_x

pytestmark = pytest.mark.gpu

N = O.N
SEED = hashlib.sha256(b"excess seed").digest()
AUX = hashlib.sha256(b"excess aux").digest()
OK, MISMATCH, MALFORMED, NOT_CANONICAL, BAD_R, NO_KEY = 0, 1, 2, 3, 4, 5
NAMES = ["32bit", "bin_test", "rec_test", "nine"]
SUB = RP.TALLY_SUBTRACT
SIG = RP.EXCESS_SIG_BYTES


@pytest.fixture(scope="module")
def handles(gpu, oracle_lib):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _native(gpu, _case(oracle_lib, name)[0])
        return made[name]
    yield get
    for nat in made.values():
        nat.close()


@pytest.fixture
def hooks():
    """the three thresholds of the shared sum stage on one handle, restored afterwards"""
    tl, touched = capi.load_test_library(), []

    def apply(nat, short_max, piece, chunk):
        assert tl.bppp_test_rp_set_tally_short_max(nat.h, short_max) == 0 and tl.bppp_test_rp_set_tally_piece(nat.h, piece) == 0
        assert tl.bppp_test_rp_set_tally_chunk(nat.h, chunk) == 0

    def set_(nat, short_max=0, piece=0, chunk=0):
        if nat not in touched:
            touched.append(nat)
        apply(nat, short_max, piece, chunk)
    yield set_
    for nat in touched:
        apply(nat, 0, 0, 0)


def _pool(oracle_lib, name):
    st, inputs, triples, pts, files = _case(oracle_lib, name)
    return st, inputs, [t for row in triples for t in row], [p for row in pts for p in row], files


def _csr(sums):
    sum_start, entries = [0], []
    for s in sums:
        entries += [RP.tally_entry(j, sub) for j, sub in s]
        sum_start.append(len(entries))
    return sum_start, entries


def _random_sums(total, lengths, seed, avoid=()):
    rng = random.Random(seed)
    pick = [j for j in range(total) if j not in avoid]
    return [[(rng.choice(pick), rng.random() < 0.4) for _ in range(n)] for n in lengths]


def _msgs(n, salt=b""):
    return [hashlib.sha256(b"excess msg %d " % t + salt).digest() for t in range(n)]


def _s_of(sig):
    return sum(int.from_bytes(sig[33 + 8 * i:41 + 8 * i], "big") << (64 * i) for i in range(4))


def _with_s(sig, s):
    return sig[:33] + RP._put(s)


def _split(host_claims):
    """tally_claims_host's (a, ty, e) per sum -> the public claims (a, ty) and the blinding sums"""
    return [(a, ty) for a, ty, _ in host_claims], [e for _, _, e in host_claims]


def _host_verdicts(be, st, flat, ss, en, public, msgs, sigs, broken=()):
    S = RP.tally_sums(be, flat, ss, en)
    return [RP.excess_verify_host(be, st, S[t], public[t], msgs[t], sigs[t], b"", malformed=any((e & (SUB - 1)) in broken for e in en[ss[t]:ss[t + 1]]))
            for t in range(len(ss) - 1)]


class _Dev:
    """pool, CSR arrays, public claims, messages and signatures of one call in HBM; alloc: another allocator than the handle's context
    (tests/guard_arena.py)"""

    def __init__(self, nat, files, sum_start, entries, public, msgs, sigs, alloc=None):
        g = self.gpu = alloc or nat.gpu
        self.rows, self.nsums, self.nnz = len(files), len(sum_start) - 1, len(entries)
        ss, en, _, _ = nat._tally_csr(sum_start, entries)
        amt, typ = nat._excess_claim_arrays(public, self.nsums)
        self.d = {"cf": g.to_device(np.frombuffer(b"".join(files), dtype=np.uint8)), "ss": g.to_device(ss), "en": g.to_device(en),
                  "amt": g.to_device(amt) if amt is not None else 0, "typ": g.to_device(typ) if typ is not None else 0,
                  "mg": g.to_device(np.frombuffer(b"".join(msgs), dtype=np.uint8)), "sg": g.to_device(np.frombuffer(b"".join(sigs), dtype=np.uint8))}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.d.values():
            if p:
                self.gpu.free(p)

    def args(self):
        d = self.d
        return self.rows, d["cf"], self.nsums, d["ss"], d["en"], self.nnz, d["amt"], d["typ"], d["mg"], d["sg"]


def _each_both(nat, files, ss, en, public, msgs, sigs):
    """verify_each with points, host and _device: the two must agree"""
    host = nat.excess_verify_each(files, ss, en, public, msgs, sigs, want_points=True)
    with _Dev(nat, files, ss, en, public, msgs, sigs) as dev:
        assert nat.excess_verify_each_device(*dev.args(), want_points=True) == host
    return host


# ----------------------------------------------------------------------------- 1. sign = the host restatement, byte for byte
@pytest.mark.parametrize("name", NAMES)
def test_sign_equals_host(gpu, oracle_lib, handles, name):
    st = _case(oracle_lib, name)[0]
    nat, be = handles(name), OracleBackend(oracle_lib)
    rng = random.Random(11)
    es = [rng.randrange(1, N) for _ in range(6)] + [1, 2, N - 1, 2**255, 2**128]
    msgs = _msgs(len(es))
    want = [RP.excess_sign_host(be, st, e, m, AUX, b"") for e, m in zip(es, msgs)]
    assert all(w[0] == 0 for w in want)
    got = nat.excess_sign(es, msgs, AUX, want_status=True, want_points=True)
    assert got == ([w[1] for w in want], [0] * len(es), [w[2] for w in want])
    assert nat.excess_sign(es, msgs, AUX) == got[0]                                   # deterministic, and no status array needed when all sign
    g = nat.gpu
    d = [g.to_device(capi.scalars_to_array(es)), g.to_device(np.frombuffer(b"".join(msgs), dtype=np.uint8)), g.to_device(np.full(len(es) * SIG, 0xA5, dtype=np.uint8))]
    try:
        assert nat.excess_sign_device(len(es), *d, AUX, want_status=True, want_points=True) == (got[1], got[2])
        raw = g.download(d[2], (len(es) * SIG,), np.uint8).tobytes()
        assert [raw[t * SIG:(t + 1) * SIG] for t in range(len(es))] == got[0]
    finally:
        for p in d:
            g.free(p)
    other = nat.excess_sign(es[:2], msgs[:2], bytes(32))
    assert all(a[:33] != b[:33] for a, b in zip(other, got[0]))                        # another aux: another nonce, another R
    # refusals: zero rows, the others signed as before
    es2, msgs2 = [es[0], 0, N, es[3], 2**256 - 1], [msgs[0], msgs[1], msgs[2], msgs[3], msgs[4]]
    sigs2, status2, pts2 = nat.excess_sign(es2, msgs2, AUX, want_status=True, want_points=True)
    assert status2 == [0, capi.RP_EXCESS_ZERO, capi.RP_EXCESS_NOT_CANONICAL, 0, capi.RP_EXCESS_NOT_CANONICAL]
    assert sigs2 == [got[0][0], bytes(SIG), bytes(SIG), got[0][3], bytes(SIG)] and pts2 == [got[2][0], None, None, got[2][3], None]
    assert [RP.excess_sign_host(be, st, e, m, AUX, b"")[0] for e, m in zip(es2, msgs2)] == status2
    with pytest.raises(capi.BpppError, match=r"rp_excess_sign: sum 1: .*zero"):
        nat.excess_sign(es2, msgs2, AUX)
    with pytest.raises(capi.BpppError, match=r"rp_excess_sign: sum 2: .*not canonical"):
        nat.excess_sign([es[0], es[1], N], msgs2[:3], AUX)
    assert nat.excess_sign([], [], AUX) == []


# ----------------------------------------------------------------------------- 2. round trip through the real job, across chunk borders
@pytest.mark.parametrize("name", NAMES)
def test_round_trip(gpu, oracle_lib, handles, hooks, name):
    st, inputs, triples, flat, files = _pool(oracle_lib, name)
    nat = handles(name)
    sums = _random_sums(len(flat), [1, 2, 3, 16, 17, 64, 65, 257], 21)
    ss, en = _csr(sums)
    claims = nat.tally_claims(inputs, ss, en)
    assert [tuple(c) for c in claims] == [((a, e) if name == "bin_test" else (a, ty, e)) for a, ty, e in RP.tally_claims_host(triples, ss, en)]
    public, blinds = [tuple(c[:-1]) for c in claims], [c[-1] for c in claims]
    msgs = _msgs(len(sums))
    sigs, _, keys = nat.excess_sign(blinds, msgs, AUX, want_status=True, want_points=True)
    good = ([OK] * len(sums), keys)
    assert None not in keys
    assert _each_both(nat, files, ss, en, public, msgs, sigs) == good
    assert nat.excess_verify_batch(files, ss, en, public, msgs, sigs, SEED, want_status=True, want_point=True) == (True, good[0], None)
    assert nat.excess_verify_batch(files, ss, en, public, msgs, sigs) is True            # a fresh seed
    # one lane up to 3 entries, pieces of 5, passes of 7 sums and entries: sums, messages and signatures cross the borders of the passes
    hooks(nat, short_max=3, piece=5, chunk=7)
    assert _each_both(nat, files, ss, en, public, msgs, sigs) == good
    assert nat.excess_verify_batch(files, ss, en, public, msgs, sigs, SEED, want_status=True, want_point=True) == (True, good[0], None)
    bad = list(sigs)
    bad[5] = _with_s(sigs[5], (_s_of(sigs[5]) + 1) % N)                                # in a later pass, a sum of its own pass
    want = [MISMATCH if t == 5 else OK for t in range(len(sums))]
    assert nat.excess_verify_each(files, ss, en, public, msgs, bad) == want
    acc, status, point = nat.excess_verify_batch(files, ss, en, public, msgs, bad, SEED, want_status=True, want_point=True)
    assert not acc and status == want and point is not None
    hooks(nat)
    assert nat.excess_verify_batch(files, ss, en, public, msgs, bad, SEED, want_point=True) == (False, None, point)


# ----------------------------------------------------------------------------- 3. verdicts = the host restatement, one defect a sum
@pytest.mark.parametrize("name", ["rec_test", "bin_test"])
def test_verdicts_equal_host(gpu, oracle_lib, handles, name):
    st, inputs, triples, flat, files = _pool(oracle_lib, name)
    nat, be, typed = handles(name), OracleBackend(oracle_lib), name != "bin_test"
    nr = len(st.rds)
    broken_j = 2 * nr + min(1, nr - 1)
    defects = ["s+1", "s>=n", "sign flipped", "sign 2", "R.x no point", "message", "amount", "entry swapped", "malformed", "no key", "malformed and bad R"]
    if typed:
        defects += ["type", "type>=n"]
    nsums = 2 * len(defects) + 1                                                       # clean sums between the defects and at both ends
    sums = _random_sums(len(flat), [3] * nsums, 31, avoid=(broken_j,))
    at = {d: 2 * i + 1 for i, d in enumerate(defects)}
    sums[at["no key"]] = [(0, False), (0, True)]
    sums[at["malformed"]][1] = (broken_j, True)
    sums[at["malformed and bad R"]][0] = (broken_j, False)
    ss, en = _csr(sums)
    host_claims = RP.tally_claims_host(triples, ss, en)
    public, blinds = _split(host_claims)
    assert host_claims[at["no key"]] == (0, 0, 0)
    blinds[at["no key"]] = 1                                                           # any signature: there is no key to check it under
    msgs = _msgs(nsums)
    sigs = nat.excess_sign(blinds, msgs, AUX)
    if not typed:
        public = [(a,) for a, _ in public]
    assert nat.excess_verify_each(files, ss, en, public, msgs, sigs) == [NO_KEY if t == at["no key"] else OK for t in range(nsums)]

    def put(seq, d, f):
        seq[at[d]] = f(seq[at[d]])
    bx = _no_point_x(oracle_lib)
    put(sigs, "s+1", lambda g: _with_s(g, (_s_of(g) + 1) % N))
    put(sigs, "s>=n", lambda g: _with_s(g, N))
    put(sigs, "sign flipped", lambda g: g[:32] + bytes([g[32] ^ 1]) + g[33:])
    put(sigs, "sign 2", lambda g: g[:32] + b"\x02" + g[33:])
    put(sigs, "R.x no point", lambda g: RP._put(bx) + g[32:])
    put(sigs, "malformed and bad R", lambda g: g[:32] + b"\x07" + g[33:])
    put(msgs, "message", lambda m: m[:-1] + bytes([m[-1] ^ 1]))
    put(public, "amount", lambda c: ((c[0] + 1) % N,) + tuple(c[1:]))
    if typed:
        put(public, "type", lambda c: (c[0], (c[1] + 1) % N))
        put(public, "type>=n", lambda c: (c[0], N))
    p = ss[at["entry swapped"]] + 1
    en[p] = RP.tally_entry(((en[p] & (SUB - 1)) + 1) % len(flat) if ((en[p] & (SUB - 1)) + 1) % len(flat) != broken_j else 0, bool(en[p] & SUB))
    broken = list(files)
    broken[2] = _set_x(files[2], nr, min(1, nr - 1), bx)
    expect = {"s+1": MISMATCH, "s>=n": NOT_CANONICAL, "sign flipped": MISMATCH, "sign 2": BAD_R, "R.x no point": BAD_R, "message": MISMATCH, "amount": MISMATCH,
              "entry swapped": MISMATCH, "malformed": MALFORMED, "no key": NO_KEY, "malformed and bad R": MALFORMED, "type": MISMATCH, "type>=n": NOT_CANONICAL}
    want = [OK] * nsums
    for d in defects:
        want[at[d]] = expect[d]
    assert _host_verdicts(be, st, flat, ss, en, public, msgs, sigs, broken=(broken_j,)) == want
    status, keys = _each_both(nat, broken, ss, en, public, msgs, sigs)
    assert status == want
    assert keys[at["malformed"]] is None and keys[at["no key"]] is None and keys[0] == oracle_lib.mul(blinds[0], st.hs[1] if typed else st.hs[0])
    acc, bstatus, _ = nat.excess_verify_batch(broken, ss, en, public, msgs, sigs, SEED, want_status=True)
    assert not acc and bstatus == want


# ----------------------------------------------------------------------------- 4. crafted equations: the branches of the complete law
@pytest.mark.parametrize("name", ["rec_test", "bin_test"])
def test_crafted_equations(gpu, oracle_lib, handles, name):
    st, inputs, _, _, _ = _case(oracle_lib, name)
    nat, be, typed = handles(name), OracleBackend(oracle_lib), name != "bin_test"
    B = st.hs[1] if typed else st.hs[0]
    rows = [list(r) for r in inputs[:2]]
    rows[0][0] = tuple(rows[0][0][:-1]) + (1,)                                          # blinding 1: the excess of this commitment over its claim is B
    files = nat.commit_batch(rows)
    trip = [[(v, 0, bl) for v, bl in r] for r in rows] if not typed else rows
    flat = [p for r in trip for p in _ref_points(oracle_lib, st, r)]
    v, ty = trip[0][0][0] % N, trip[0][0][1]
    public = [(v, ty) if typed else (v,)] * 4
    ss, en = _csr([[(0, False)]] * 4)
    msgs = _msgs(4, b"crafted")
    sigs = nat.excess_sign([1, 1, 1, 1], msgs, AUX)
    c = [RP.excess_challenge(b"", g[:33], B, m) for g, m in zip(sigs, msgs)]
    sigs[1] = _with_s(sigs[1], N - c[1])                                               # c X and - s B are the same point: the doubling branch
    sigs[2] = _with_s(sigs[2], c[2])                                                   # s B - c X is infinity
    sigs[3] = _with_s(sigs[3], 0)                                                      # s B is infinity
    want = [OK, MISMATCH, MISMATCH, MISMATCH]
    assert _host_verdicts(be, st, flat, ss, en, public, msgs, sigs) == want
    assert _each_both(nat, files, ss, en, public, msgs, sigs) == (want, [B] * 4)
    acc, status, _ = nat.excess_verify_batch(files, ss, en, public, msgs, sigs, SEED, want_status=True)
    assert not acc and status == want


# ----------------------------------------------------------------------------- 5. the quad walk alone against the oracle's scalar multiplication
def test_quad_walk_equals_oracle(gpu, oracle_lib, handles):
    st, _, _, flat, _ = _pool(oracle_lib, "rec_test")
    nat, ec, tl = handles("rec_test"), oracle_lib, capi.load_test_library()
    rng = random.Random(5)
    scalars = [0, 1, 2, 3, N - 1, N - 2, 2**255, 2**256 - 1] + [2**k for k in (31, 32, 64, 129, 254)] + [2**k - 1 for k in (32, 33, 128, 255)]
    scalars += [rng.randrange(2**256) for _ in range(16)]
    points = [st.g, st.hs[0], st.hs[1], flat[7], None]
    pairs = [(c, p) for c in scalars for p in points]
    rng.shuffle(pairs)
    want = [None if p is None or c % N == 0 else ec.mul(c % N, p) for c, p in pairs]
    g = nat.gpu
    lo = 0
    for count in (1, 15, 16, 17, 65, len(pairs) - 114):                                # partial wavefronts and partial last quads; every pair once
        part = pairs[lo:lo + count]
        d = [g.to_device(capi.scalars_to_array([c for c, _ in part])), g.to_device(capi.points_to_array([p for _, p in part])), g.alloc(64 * count)]
        try:
            assert tl.bppp_test_rp_excess_mul(nat.h, count, *d) == 0
            out = g.download(d[2], (count, 8), np.uint64)
        finally:
            for q in d:
                g.free(q)
        assert [capi.array_to_point(out[i]) for i in range(count)] == want[lo:lo + count], count
        lo += count
    assert lo == len(pairs)


# ----------------------------------------------------------------------------- 6. the weighted combination
@pytest.mark.parametrize("name", ["rec_test", "bin_test"])
def test_batch(gpu, oracle_lib, handles, name):
    st, inputs, triples, flat, files = _pool(oracle_lib, name)
    nat, be, ec, typed = handles(name), OracleBackend(oracle_lib), oracle_lib, name != "bin_test"
    B = st.hs[1] if typed else st.hs[0]
    sums = _random_sums(len(flat), [4, 3, 1, 20, 1, 2, 40, 5], 41)
    ss, en = _csr(sums)
    public, blinds = _split(RP.tally_claims_host(triples, ss, en))
    if not typed:
        public = [(a,) for a, _ in public]
    msgs = _msgs(len(sums), b"batch")
    sigs, _, keys = nat.excess_sign(blinds, msgs, AUX, want_status=True, want_points=True)
    acc, status, point = nat.excess_verify_batch(files, ss, en, public, msgs, sigs, SEED, want_status=True, want_point=True)
    assert acc and status == [OK] * len(sums) and point is None
    assert nat.excess_verify_batch(files, ss, en, public, msgs, sigs, hashlib.sha256(b"another").digest(), want_point=True) == (True, None, None)
    bad_sigs, bad_msgs = list(sigs), list(msgs)
    bad_sigs[3] = _with_s(sigs[3], (_s_of(sigs[3]) + 1) % N)
    bad_msgs[6] = msgs[6][::-1]

    def lift(sig):
        x = RP.decode_field(sig[:32], RP.FIELD_P)
        y = ec.lift_x(x)[1]
        return (x, y if (y > RP.FIELD_P - y) == bool(sig[32]) else RP.FIELD_P - y)

    def combined(seed, offset, lo, hi):
        """sum over t in [lo, hi) of rho_t (s_t B - c_t X_t - R_t), by the oracle"""
        terms = []
        for t in range(lo, hi):
            rho = RP.excess_weight(seed, offset + t, bad_sigs[t], keys[t], bad_msgs[t])
            c = RP.excess_challenge(b"", bad_sigs[t][:33], keys[t], bad_msgs[t])
            terms += [(rho * _s_of(bad_sigs[t]) % N, B), ((-rho * c) % N, keys[t]), ((-rho) % N, lift(bad_sigs[t]))]
        return ec.inner_product(terms)
    want = combined(SEED, 0, 0, len(sums))
    each = nat.excess_verify_each(files, ss, en, public, bad_msgs, bad_sigs)
    assert each == [MISMATCH if t in (3, 6) else OK for t in range(len(sums))]
    acc, status, point = nat.excess_verify_batch(files, ss, en, public, bad_msgs, bad_sigs, SEED, want_status=True, want_point=True)
    assert not acc and status == each and point == want and point is not None
    other = nat.excess_verify_batch(files, ss, en, public, bad_msgs, bad_sigs, hashlib.sha256(b"another").digest(), want_point=True)
    assert other[0] is False and other[2] not in (None, want)
    # host = _device; three shards of one job add up to the one-call point; another offset is another point
    with _Dev(nat, files, ss, en, public, bad_msgs, bad_sigs) as dev:
        assert nat.excess_verify_batch_device(*dev.args(), seed=SEED, want_status=True, want_point=True) == (False, each, want)
        acc7, _, p7 = nat.excess_verify_batch_device(*dev.args(), seed=SEED, index_offset=2**32 + 7, want_point=True)
        assert not acc7 and p7 == combined(SEED, 2**32 + 7, 0, len(sums)) and p7 != want
    parts = []
    for lo, hi in ((0, 3), (3, 6), (6, len(sums))):
        ssk = [v - ss[lo] for v in ss[lo:hi + 1]]
        with _Dev(nat, files, ssk, en[ss[lo]:ss[hi]], public[lo:hi], bad_msgs[lo:hi], bad_sigs[lo:hi]) as dk:
            ak, _, pk = nat.excess_verify_batch_device(*dk.args(), seed=SEED, index_offset=lo, want_point=True)
        assert pk == combined(SEED, 0, lo, hi) and ak == (lo == 0)
        parts.append(pk)
    assert parts[0] is None and gpu.sum_points(capi.points_to_array(parts)) == want
    # the empty job
    acc0 = C.c_int(-1)
    assert gpu.lib.bppp_rp_excess_verify_batch_device(nat.h, 0, None, 0, None, None, 0, None, None, None, None, 9, None, C.byref(acc0), None, None) == 0 and acc0.value == 1
    assert gpu.lib.bppp_rp_excess_verify_each(nat.h, 0, None, 0, None, None, 0, None, None, None, None, None, None) == 0


# ----------------------------------------------------------------------------- 7. argument errors, as the tally's
def test_errors(gpu, oracle_lib, handles):
    st, inputs, triples, flat, files = _pool(oracle_lib, "rec_test")
    nat, lib, total = handles("rec_test"), gpu.lib, len(flat)
    sums = [[(1, False), (2, True)], [(3, False)], [(4, False), (5, False), (6, True)]]
    ss, en = _csr(sums)
    public, blinds = _split(RP.tally_claims_host(triples, ss, en))
    msgs = _msgs(3)
    sigs = nat.excess_sign(blinds, msgs, AUX)
    for bad_ss, bad_en, msg in (([0, 2, 1, 6], en, r"rp_excess_verify_\w+: sum_start\[2\] = 1 "),
                                (ss, en[:4] + [total | SUB] + en[5:], r"rp_excess_verify_\w+: entries\[4\]: index %d " % total)):
        with pytest.raises(capi.BpppError, match=msg):
            nat.excess_verify_each(files, bad_ss, bad_en, public, msgs, sigs)
        with pytest.raises(capi.BpppError, match=msg):
            nat.excess_verify_batch(files, bad_ss, bad_en, public, msgs, sigs, SEED)
    with _Dev(nat, files, ss, en, public, msgs, sigs) as dev:
        a = dev.args()
        p = [C.c_void_p(v) for v in a]
        status, acc = np.full(3, 0xA5A5A5A5, dtype=np.uint32), C.c_int(-1)
        vp = lambda x: C.c_void_p(x.ctypes.data)
        for k in (6, 7):                                                               # only one of the two claim arrays
            q = list(p)
            q[k] = None
            assert lib.bppp_rp_excess_verify_each_device(nat.h, a[0], q[1], 3, q[3], q[4], 6, q[6], q[7], q[8], q[9], vp(status), None) == -1
            assert b"claim_" in lib.bppp_last_error(gpu.h)
        for k in (1, 3, 8, 9):                                                         # NULL buffers
            q = list(p)
            q[k] = None
            assert lib.bppp_rp_excess_verify_each_device(nat.h, a[0], q[1], 3, q[3], q[4], 6, q[6], q[7], q[8], q[9], vp(status), None) == -1
            assert b"null input" in lib.bppp_last_error(gpu.h)
        assert lib.bppp_rp_excess_verify_each_device(nat.h, a[0], p[1], 3, p[3], p[4], 6, p[6], p[7], p[8], p[9], None, None) == -1
        assert lib.bppp_rp_excess_verify_batch_device(nat.h, a[0], p[1], 3, p[3], p[4], 6, p[6], p[7], p[8], p[9], 0, None, C.byref(acc), None, None) == -1
        assert (status == 0xA5A5A5A5).all() and acc.value == 0
        assert lib.bppp_rp_excess_verify_each_device(nat.h, a[0], p[1], 3, p[3], p[4], 6, None, None, p[8], p[9], vp(status), None) == 0       # zero claims
        assert list(status) == [MISMATCH] * 3
    assert lib.bppp_rp_excess_sign(nat.h, 1, None, None, None, None, None, None) == -1 and b"null input" in lib.bppp_last_error(gpu.h)


# ----------------------------------------------------------------------------- 8. the handle's workspace is shared: a plain tally is unchanged
def test_plain_tally_is_unchanged(gpu, oracle_lib, handles):
    st, inputs, triples, flat, files = _pool(oracle_lib, "nine")
    nat = handles("nine")
    sums = _random_sums(len(flat), [3, 0, 17, 1, 70, 5], 51)
    ss, en = _csr(sums)
    claims = RP.tally_claims_host(triples, ss, en)
    claims[3] = ((claims[3][0] + 1) % N, claims[3][1], claims[3][2])
    before = (nat.tally_each(files, ss, en, claims, want_points=True), nat.tally_batch(files, ss, en, claims, SEED, want_status=True, want_point=True))
    assert before[0][0] == [MISMATCH if t == 3 else OK for t in range(len(sums))]
    public, blinds = _split(RP.tally_claims_host(triples, ss, en))
    blinds[1] = 1
    msgs = _msgs(len(sums))
    sigs = nat.excess_sign(blinds, msgs, AUX)
    want = [NO_KEY if t == 1 else OK for t in range(len(sums))]
    assert nat.excess_verify_each(files, ss, en, public, msgs, sigs) == want
    assert nat.excess_verify_batch(files, ss, en, public, msgs, sigs, SEED, want_status=True)[:2] == (False, want)
    after = (nat.tally_each(files, ss, en, claims, want_points=True), nat.tally_batch(files, ss, en, claims, SEED, want_status=True, want_point=True))
    assert after == before
