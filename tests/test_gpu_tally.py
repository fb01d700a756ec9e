"""bppp_rp_tally_each*, bppp_rp_tally_batch*, bppp_rp_tally_claims*: signed sums of commitments against claimed openings.

The reference side is the host protocol code over the oracle backend (tests/rp_backends.py): rangeproof.tally_sums adds and subtracts the
reference commitments of test_gpu_commit_open's 65 rows with the oracle's group law, rangeproof.tally_claims_host adds their witnesses as plain
integers, rangeproof.tally_weight restates the weight — never the library under test.  The pools and their reference points are computed once
per setup (test_gpu_commit_open._case) and shared."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from rp_backends import OracleBackend
from test_gpu_commit_open import ROWS, _case, _native, _no_point_x, _set_x

pytestmark = pytest.mark.gpu

N = O.N
SEED = hashlib.sha256(b"tally seed").digest()
ERR_ARG = -1
OK, MISMATCH, MALFORMED, NOT_CANONICAL = 0, 1, 2, 3
NAMES = ["32bit", "bin_test", "rec_test", "nine"]
SUB = RP.TALLY_SUBTRACT


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
    """the three thresholds of one handle, restored afterwards"""
    tl, touched = capi.load_test_library(), []

    def apply(nat, short_max, piece, chunk):
        assert tl.bppp_test_rp_set_tally_short_max(nat.h, short_max) == 0 and tl.bppp_test_rp_set_tally_piece(nat.h, piece) == 0
        assert tl.bppp_test_rp_set_tally_chunk(nat.h, chunk) == 0

    def set_(nat, short_max=0, piece=0, chunk=0):
        if nat not in touched:
            touched.append(nat)
        apply(nat, short_max, piece, chunk)
    yield set_
    for nat in touched:                    # 0 restores a default; `touched` does not grow here
        apply(nat, 0, 0, 0)


def _pool(oracle_lib, name):
    """(setup, witness rows, flat (v, ty, bl) triples, flat reference points, files) of the 65 rows"""
    st, inputs, triples, pts, files = _case(oracle_lib, name)
    return st, inputs, [t for row in triples for t in row], [p for row in pts for p in row], files


def _csr(sums):
    """sums = [[(flat index, subtract)]] -> sum_start, entries"""
    sum_start, entries = [0], []
    for s in sums:
        entries += [RP.tally_entry(j, sub) for j, sub in s]
        sum_start.append(len(entries))
    return sum_start, entries


def _random_sums(total, lengths, seed):
    rng = random.Random(seed)
    return [[(rng.randrange(total), rng.random() < 0.4) for _ in range(n)] for n in lengths]


def _claims_for(nat, claims):
    return [(a, e) for a, _, e in claims] if isinstance(nat, BRP.NativeBinaryRangeProofs) else claims


def _claim_point(ec, st, claim):
    a, ty, e = claim
    if isinstance(st, BRP.SetupBRP):
        return ec.inner_product([(a % N, st.g), (e % N, st.hs[0])])
    return ec.inner_product([(a % N, st.g), (ty % N, st.hs[0]), (e % N, st.hs[1])])


class _Dev:
    """pool, CSR arrays and claims of one call in HBM; alloc: another allocator than the handle's context (tests/guard_arena.py)"""

    def __init__(self, nat, files, sum_start, entries, claims=None, alloc=None):
        g = self.gpu = alloc or nat.gpu
        self.rows, self.nsums, self.nnz = len(files), len(sum_start) - 1, len(entries)
        ss, en, _, _ = nat._tally_csr(sum_start, entries)
        amt, typ, bld = nat._tally_claim_arrays(claims, self.nsums)
        binary = isinstance(nat, BRP.NativeBinaryRangeProofs)
        self.d = {"cf": g.to_device(np.frombuffer(b"".join(files), dtype=np.uint8)), "ss": g.to_device(ss), "en": g.to_device(en),
                  "amt": g.to_device(amt) if claims is not None else 0, "typ": g.to_device(typ) if claims is not None and not binary else 0,
                  "bld": g.to_device(bld) if claims is not None else 0}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.d.values():
            if p:
                self.gpu.free(p)

    def args(self):
        d = self.d
        return self.rows, d["cf"], self.nsums, d["ss"], d["en"], self.nnz, d["amt"], d["typ"], d["bld"]


def _each_both(nat, files, sum_start, entries, claims=None):
    """tally_each with points, host and _device: the two must agree"""
    host = nat.tally_each(files, sum_start, entries, claims, want_points=True)
    with _Dev(nat, files, sum_start, entries, claims) as dev:
        assert nat.tally_each_device(*dev.args(), want_points=True) == host
    return host


# ----------------------------------------------------------------------------- 1. sums = reference, across both thresholds and several pieces
@pytest.mark.parametrize("name", NAMES)
def test_sums_equal_reference(gpu, oracle_lib, handles, hooks, name):
    st, _, _, flat, files = _pool(oracle_lib, name)
    nat, be = handles(name), OracleBackend(oracle_lib)
    # the defaults: one lane up to 16 entries, one workgroup beyond; 257 = one lane past the workgroup's first stride
    lengths = [0, 1, 2, 3, 63, 64, 65, 257, 16, 17]
    ss, en = _csr(_random_sums(len(flat), lengths, 1))
    want = RP.tally_sums(be, flat, ss, en)
    status, points = _each_both(nat, files, ss, en)
    assert points == want and status == [OK if p is None else MISMATCH for p in want] and status[0] == OK
    # one lane up to 3 entries, pieces of 5: at, below and above both; 13 = three pieces, 26 = six pieces whose partial points are split again
    hooks(nat, short_max=3, piece=5)
    lengths = [2, 3, 4, 5, 6, 13, 26, 0, 1]
    ss, en = _csr(_random_sums(len(flat), lengths, 2))
    want = RP.tally_sums(be, flat, ss, en)
    status, points = _each_both(nat, files, ss, en)
    assert points == want and status == [OK if p is None else MISMATCH for p in want]
    hooks(nat, short_max=1, piece=2)                                                  # the narrowest tree: 13 entries through four levels
    assert nat.tally_each(files, ss, en, want_points=True) == (status, points)


# ----------------------------------------------------------------------------- 2. the corners of the group law
def test_group_law_corners(gpu, oracle_lib, handles):
    st, _, triples, flat, files = _pool(oracle_lib, "rec_test")
    nat, be = handles("rec_test"), OracleBackend(oracle_lib)
    j, k, m = 7, 100, len(flat) - 1
    sums = [[(j, False), (j, False), (k, False)],                                     # the same index twice in a row: a doubling on the short route
            [(k, False), (j, False), (j, True), (m, False)],                          # + j - j in the middle: through the identity and out again
            [(j, False), (k, True), (j, True), (k, False)],                           # cancels to the identity
            [(j, False)] * 128,                                                       # long route, one entry a lane: every tree addition is a doubling
            [(j, True), (k, True), (m, True)],                                        # subtracted entries only
            [(j, False), (j, True)] * 64 + [(k, False)]]                              # long route: lanes that hold P and lanes that hold - P
    ss, en = _csr(sums)
    want = RP.tally_sums(be, flat, ss, en)
    assert want[2] is None and want[3] == oracle_lib.mul(128, flat[j]) and want[5] == flat[k]
    claims = RP.tally_claims_host(triples, ss, en)
    assert claims[2] == (0, 0, 0)
    status, points = _each_both(nat, files, ss, en, claims)
    assert points == want and status == [OK] * len(sums)
    status, points = _each_both(nat, files, ss, en)                                   # zero claims: only the cancelling sum balances to nothing
    assert points == want and status == [MISMATCH, MISMATCH, OK, MISMATCH, MISMATCH, MISMATCH]
    wrong = list(claims)
    wrong[2] = (1, 0, 0)                                                              # the identity against a non-zero claim
    assert nat.tally_each(files, ss, en, wrong) == [OK, OK, MISMATCH, OK, OK, OK]


# ----------------------------------------------------------------------------- 3. tally_claims round trip
@pytest.mark.parametrize("name", ["rec_test", "bin_test", "nine"])
def test_tally_claims_round_trip(gpu, oracle_lib, handles, name):
    st, inputs, triples, flat, files = _pool(oracle_lib, name)
    nat, binary = handles(name), name == "bin_test"
    assert nat.commit_batch(inputs) == files
    lengths = [4, 0, 1, 2, 16, 17, 5, 70]
    sums = _random_sums(len(flat), lengths, 3)
    ss, en = _csr(sums)
    claims = nat.tally_claims(inputs, ss, en)
    assert claims == _claims_for(nat, RP.tally_claims_host(triples, ss, en))
    good = [OK] * len(sums)
    assert nat.tally_each(files, ss, en, claims) == good
    # the _device form writes the arrays the other entry points take
    amt, typ, bld = nat._claim_arrays(inputs)
    g = nat.gpu
    with _Dev(nat, files, ss, en) as dev:
        d_in = [g.to_device(amt), 0 if binary else g.to_device(typ), g.to_device(bld)]
        d_out = [g.alloc(32 * len(sums)), 0 if binary else g.alloc(32 * len(sums)), g.alloc(32 * len(sums))]
        try:
            nat.tally_claims_device(ROWS, *d_in, dev.nsums, dev.d["ss"], dev.d["en"], dev.nnz, *d_out)
            assert nat.tally_each_device(ROWS, dev.d["cf"], dev.nsums, dev.d["ss"], dev.d["en"], dev.nnz, *d_out) == good
            assert nat.tally_batch_device(ROWS, dev.d["cf"], dev.nsums, dev.d["ss"], dev.d["en"], dev.nnz, *d_out, seed=SEED) is True
        finally:
            for p in d_in + d_out:
                if p:
                    g.free(p)
    t = 4

    def only(code):
        return [code if i == t else OK for i in range(len(sums))]

    def changed(f):
        out = list(claims)
        out[t] = f(out[t])
        return out
    assert nat.tally_each(files, ss, en, changed(lambda c: ((c[0] + 1) % N,) + tuple(c[1:]))) == only(MISMATCH)
    assert nat.tally_each(files, ss, en, changed(lambda c: tuple(c[:-1]) + ((c[-1] + 1) % N,))) == only(MISMATCH)
    assert nat.tally_each(files, ss, en, changed(lambda c: (c[0] - N,) + tuple(c[1:]))) == good           # an amount is an integer reduced mod n
    flipped = list(en)
    flipped[ss[t] + 3] ^= SUB
    assert nat.tally_each(files, ss, flipped, claims) == only(MISMATCH)
    # a witness that is no scalar: the lowest sum that references it is named
    bad_inputs = [list(r) for r in inputs]
    row, i = divmod(sums[t][0][0], len(st.rds))
    bad_inputs[row][i] = tuple(bad_inputs[row][i][:-1]) + (N,)
    first = min(s for s, entries in enumerate(sums) if sums[t][0][0] in [j for j, _ in entries])
    with pytest.raises(capi.BpppError, match=r"sum %d: .*not canonical" % first):
        nat.tally_claims(bad_inputs, ss, en)


# ----------------------------------------------------------------------------- 4. precedence: the file before the claim, and only what is referenced
def test_precedence(gpu, oracle_lib, handles):
    st, inputs, triples, flat, files = _pool(oracle_lib, "rec_test")
    nat, nr = handles("rec_test"), len(st.rds)
    broken_j = 2 * nr + 1
    broken = list(files)
    broken[2] = _set_x(files[2], nr, 1, _no_point_x(oracle_lib))
    sums = [[(0, False), (broken_j, True)], [(3, False), (4, False)], [(j, False) for j in range(30)] + [(broken_j, False)], [(5, True)], []]
    ss, en = _csr(sums)
    claims = RP.tally_claims_host(triples, ss, en)
    assert nat.tally_each(files, ss, en, claims) == [OK] * 5
    status, points = _each_both(nat, broken, ss, en, claims)
    assert status == [MALFORMED, OK, MALFORMED, OK, OK] and points[0] is None and points[2] is None and points[1] is not None
    # the same defect in a commitment that no sum references changes nothing
    ss2, en2 = _csr(sums[1:2] + sums[3:])
    assert _each_both(nat, broken, ss2, en2, claims[1:2] + claims[3:]) == _each_both(nat, files, ss2, en2, claims[1:2] + claims[3:])
    assert nat.tally_batch(broken, ss2, en2, claims[1:2] + claims[3:], SEED) is True
    # MALFORMED wins over NOT_CANONICAL
    nc = list(claims)
    nc[0], nc[1] = (nc[0][0], nc[0][1], N), (nc[1][0], N, nc[1][2])
    assert nat.tally_each(broken, ss, en, nc) == [MALFORMED, NOT_CANONICAL, MALFORMED, OK, OK]
    acc, status, _ = nat.tally_batch(broken, ss, en, nc, SEED, want_status=True)
    assert not acc and status == [MALFORMED, NOT_CANONICAL, MALFORMED, OK, OK]
    # no claim arrays = explicit zeros
    assert _each_both(nat, files, ss, en) == _each_both(nat, files, ss, en, [(0, 0, 0)] * 5)
    assert nat.tally_each(files, ss, en) == [MISMATCH, MISMATCH, MISMATCH, MISMATCH, OK]


# ----------------------------------------------------------------------------- 5. the weighted combination
@pytest.mark.parametrize("name", ["rec_test", "bin_test"])
def test_batch(gpu, oracle_lib, handles, name):
    st, inputs, triples, flat, files = _pool(oracle_lib, name)
    nat, be, ec = handles(name), OracleBackend(oracle_lib), oracle_lib
    sums = _random_sums(len(flat), [4, 3, 0, 20, 1, 2, 40, 5], 5)
    ss, en = _csr(sums)
    ref = RP.tally_sums(be, flat, ss, en)
    claims = RP.tally_claims_host(triples, ss, en)
    acc, status, point = nat.tally_batch(files, ss, en, _claims_for(nat, claims), SEED, want_status=True, want_point=True)
    assert acc and status == [OK] * len(sums) and point is None
    assert nat.tally_batch(files, ss, en, _claims_for(nat, claims)) is True            # a fresh seed
    bad = list(claims)
    bad[3] = ((bad[3][0] + 1) % N, bad[3][1], bad[3][2])
    bad[6] = (bad[6][0], bad[6][1], (bad[6][2] + 5) % N)

    def combined(seed, offset, lo, hi):
        """sum over t in [lo, hi) of rho_t (S_t - claim_t), by the oracle"""
        terms = []
        for t in range(lo, hi):
            rho = RP.tally_weight(seed, offset + t, *bad[t])
            terms += [(rho, p) for p in (ref[t],) if p is not None]
            terms += [((-rho) % N, p) for p in (_claim_point(ec, st, bad[t]),) if p is not None]
        return ec.inner_product(terms) if terms else None
    want = combined(SEED, 0, 0, len(sums))
    acc, status, point = nat.tally_batch(files, ss, en, _claims_for(nat, bad), SEED, want_status=True, want_point=True)
    assert not acc and point == want and point is not None
    assert status == nat.tally_each(files, ss, en, _claims_for(nat, bad)) == [MISMATCH if t in (3, 6) else OK for t in range(len(sums))]
    # a permutation of the entries within a sum leaves the point where it is
    perm = list(en)
    perm[ss[6]:ss[7]] = reversed(en[ss[6]:ss[7]])
    perm[ss[3]:ss[4]] = en[ss[3] + 7:ss[4]] + en[ss[3]:ss[3] + 7]
    assert perm != en and nat.tally_batch(files, ss, perm, _claims_for(nat, bad), SEED, want_point=True) == (False, None, want)
    # host = _device; two shards of one job add up to the one-call point; another offset is another point
    with _Dev(nat, files, ss, en, _claims_for(nat, bad)) as dev:
        assert nat.tally_batch_device(*dev.args(), seed=SEED, want_status=True, want_point=True) == (False, status, want)
        acc7, _, p7 = nat.tally_batch_device(*dev.args(), seed=SEED, index_offset=7, want_point=True)
        assert not acc7 and p7 == combined(SEED, 7, 0, len(sums)) and p7 != want
    cut = 5
    ss0, ss1 = ss[:cut + 1], [v - ss[cut] for v in ss[cut:]]
    with _Dev(nat, files, ss0, en[:ss[cut]], _claims_for(nat, bad[:cut])) as d0, _Dev(nat, files, ss1, en[ss[cut]:], _claims_for(nat, bad[cut:])) as d1:
        a0, _, p0 = nat.tally_batch_device(*d0.args(), seed=SEED, index_offset=0, want_point=True)
        a1, _, p1 = nat.tally_batch_device(*d1.args(), seed=SEED, index_offset=cut, want_point=True)
    assert not a0 and not a1 and p0 == combined(SEED, 0, 0, cut) and p0 is not None and p1 is not None
    assert gpu.sum_points(capi.points_to_array([p0, p1])) == want


# ----------------------------------------------------------------------------- 6. argument errors: refused before anything reads through the arrays
def test_errors(gpu, oracle_lib, handles):
    st, inputs, triples, flat, files = _pool(oracle_lib, "rec_test")
    nat, lib, total = handles("rec_test"), gpu.lib, len(flat)
    sums = [[(1, False), (2, True)], [(3, False)], [(4, False), (5, False), (6, True)]]
    ss, en = _csr(sums)
    claims = RP.tally_claims_host(triples, ss, en)
    cases = [([0, 2, 1, 6], en, r"sum_start\[2\] = 1 "),                             # decreasing
             ([0, 2, 3, 5], en, r"sum_start\[3\] = 5 .*nnz = 6"),                     # the last offset is not nnz
             ([1, 2, 3, 6], en, r"sum_start\[0\] = 1 "),                              # does not start at 0
             (ss, en[:4] + [total | SUB] + en[5:], r"entries\[4\]: index %d " % total),   # an index = rows * nranges
             (ss, en[:2] + [2**31 - 1] + en[3:], r"entries\[2\]: index %d " % (2**31 - 1))]
    amt, typ, bld = nat._claim_arrays(inputs)
    g = nat.gpu
    d_wit = [g.to_device(amt), g.to_device(typ), g.to_device(bld)]
    pattern = np.full(3 * 4, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    d_out = [g.to_device(pattern) for _ in range(3)]
    try:
        for bad_ss, bad_en, msg in cases:
            with pytest.raises(capi.BpppError, match=msg):
                nat.tally_each(files, bad_ss, bad_en, claims)
            with pytest.raises(capi.BpppError, match=msg):
                nat.tally_batch(files, bad_ss, bad_en, claims, SEED)
            with pytest.raises(capi.BpppError, match=msg):
                nat.tally_claims(inputs, bad_ss, bad_en)
            with _Dev(nat, files, bad_ss, bad_en, claims) as dev:
                status, xy, acc = np.full(3, 0xA5A5A5A5, dtype=np.uint32), np.full((3, 8), 0xA5, dtype=np.uint64), C.c_int(-1)
                vp = lambda a: C.c_void_p(a.ctypes.data)
                p = [C.c_void_p(v) for v in dev.args()[1:2] + dev.args()[3:5] + dev.args()[6:]]
                assert lib.bppp_rp_tally_each_device(nat.h, ROWS, p[0], 3, p[1], p[2], 6, p[3], p[4], p[5], vp(status), vp(xy)) == ERR_ARG
                assert lib.bppp_rp_tally_batch_device(nat.h, ROWS, p[0], 3, p[1], p[2], 6, p[3], p[4], p[5], 0, SEED, C.byref(acc), vp(status), None) == ERR_ARG
                assert (status == 0xA5A5A5A5).all() and (xy == 0xA5).all() and acc.value == 0
                assert lib.bppp_last_error(gpu.h).decode().startswith("rp_tally_batch: ")
                with pytest.raises(capi.BpppError, match=msg):
                    nat.tally_claims_device(ROWS, *d_wit, 3, dev.d["ss"], dev.d["en"], 6, *d_out)
                assert all((g.download(d, (12,), np.uint64) == pattern).all() for d in d_out)
        # only one or two of the three claim arrays
        ssa, ena, _, _ = nat._tally_csr(ss, en)
        ca, ct, cb = nat._tally_claim_arrays(claims, 3)
        cf = np.frombuffer(b"".join(files), dtype=np.uint8)
        status, acc = np.full(3, 0xA5A5A5A5, dtype=np.uint32), C.c_int(-1)
        vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        for trio in ((ca, None, cb), (None, ct, cb), (ca, ct, None), (None, None, cb)):
            assert lib.bppp_rp_tally_each(nat.h, ROWS, vp(cf), 3, vp(ssa), vp(ena), 6, *map(vp, trio), vp(status), None) == ERR_ARG
            assert b"claim_" in lib.bppp_last_error(gpu.h)
            assert lib.bppp_rp_tally_batch(nat.h, ROWS, vp(cf), 3, vp(ssa), vp(ena), 6, *map(vp, trio), SEED, C.byref(acc), vp(status), None) == ERR_ARG
            with _Dev(nat, files, ss, en, claims) as dev:
                a = dev.args()
                ptrs = [C.c_void_p(v) if t is not None else None for v, t in zip(a[6:], trio)]
                assert lib.bppp_rp_tally_each_device(nat.h, ROWS, C.c_void_p(a[1]), 3, C.c_void_p(a[3]), C.c_void_p(a[4]), 6, *ptrs, vp(status), None) == ERR_ARG
                assert b"claim_" in lib.bppp_last_error(gpu.h)
        assert (status == 0xA5A5A5A5).all()
        # a binary handle's types do not count
        bst, binputs, btriples, bflat, bfiles = _pool(oracle_lib, "bin_test")
        bnat = handles("bin_test")
        bclaims = _claims_for(bnat, RP.tally_claims_host(btriples, ss, en))
        ba, _, bb = bnat._tally_claim_arrays(bclaims, 3)
        bcf = np.frombuffer(b"".join(bfiles), dtype=np.uint8)
        assert lib.bppp_rp_tally_each(bnat.h, ROWS, vp(bcf), 3, vp(ssa), vp(ena), 6, vp(ba), None, vp(bb), vp(status), None) == 0 and not status.any()
        # NULL buffers, the size limits, the empty job
        assert lib.bppp_rp_tally_each(nat.h, ROWS, vp(cf), 3, vp(ssa), vp(ena), 6, vp(ca), vp(ct), vp(cb), None, None) == ERR_ARG
        assert lib.bppp_rp_tally_each(nat.h, ROWS, None, 3, vp(ssa), vp(ena), 6, vp(ca), vp(ct), vp(cb), vp(status), None) == ERR_ARG
        assert lib.bppp_rp_tally_each(nat.h, ROWS, vp(cf), 3, None, vp(ena), 6, vp(ca), vp(ct), vp(cb), vp(status), None) == ERR_ARG
        assert lib.bppp_rp_tally_batch(nat.h, ROWS, vp(cf), 3, vp(ssa), vp(ena), 6, vp(ca), vp(ct), vp(cb), None, C.byref(acc), None, None) == ERR_ARG
        assert b"null input" in lib.bppp_last_error(gpu.h)
        assert lib.bppp_rp_tally_each(nat.h, (2**31 + 2) // 3, vp(cf), 3, vp(ssa), vp(ena), 6, vp(ca), vp(ct), vp(cb), vp(status), None) == ERR_ARG
        assert lib.bppp_rp_tally_each(nat.h, ROWS, vp(cf), 3, vp(ssa), vp(ena), 2**31, vp(ca), vp(ct), vp(cb), vp(status), None) == ERR_ARG
        assert b"2^31" in lib.bppp_last_error(gpu.h)
        assert lib.bppp_rp_tally_each(nat.h, 0, None, 0, None, None, 0, None, None, None, None, None) == 0
        assert lib.bppp_rp_tally_batch_device(nat.h, 0, None, 0, None, None, 0, None, None, None, 9, None, C.byref(acc), None, None) == 0 and acc.value == 1
        assert lib.bppp_rp_tally_claims(nat.h, 0, None, None, None, 0, None, None, 0, None, None, None) == 0
    finally:
        for p in d_wit + d_out:
            g.free(p)


def test_closed_context_is_an_argument_error(oracle_lib):
    import bulletproofspp_amd as b_
    st, inputs, _, _, files = _case(oracle_lib, "32bit")
    ctx = b_.Bppp(0)
    nat = _native(ctx, st)
    ss, en = np.array([0, 1], dtype=np.uint32), np.array([0], dtype=np.uint32)
    cf, status, acc = np.frombuffer(files[0], dtype=np.uint8).copy(), np.zeros(1, dtype=np.uint32), C.c_int(-1)
    amt, typ, bld = nat._claim_arrays(inputs[:1])
    out = np.zeros((3, 4), dtype=np.uint64)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    h = nat.h
    ctx.lib.bppp_ctx_destroy(ctx.h)                # the context is closed; the child handle keeps it alive
    ctx.h = None
    try:
        assert ctx.lib.bppp_rp_tally_each(h, 1, vp(cf), 1, vp(ss), vp(en), 1, None, None, None, vp(status), None) == ERR_ARG
        assert ctx.lib.bppp_rp_tally_batch(h, 1, vp(cf), 1, vp(ss), vp(en), 1, None, None, None, SEED, C.byref(acc), None, None) == ERR_ARG
        assert ctx.lib.bppp_rp_tally_claims(h, 1, vp(amt), vp(typ), vp(bld), 1, vp(ss), vp(en), 1, vp(out[0]), vp(out[1]), vp(out[2])) == ERR_ARG
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 7. several passes over the workspace = one
def test_chunking(gpu, oracle_lib, handles, hooks):
    st, inputs, triples, flat, files = _pool(oracle_lib, "nine")
    nat, be = handles("nine"), OracleBackend(oracle_lib)
    sums = _random_sums(len(flat), [3, 4, 0, 0, 0, 2, 20, 1, 6, 7, 0, 5], 7)           # 48 entries; 20 alone is more than a pass of 7 holds
    ss, en = _csr(sums)
    claims = RP.tally_claims_host(triples, ss, en)
    claims[8] = ((claims[8][0] + 1) % N, claims[8][1], claims[8][2])
    one = nat.tally_each(files, ss, en, claims, want_points=True)
    one_batch = nat.tally_batch(files, ss, en, claims, SEED, want_status=True, want_point=True)
    assert one[1] == RP.tally_sums(be, flat, ss, en) and one[0] == [MISMATCH if t == 8 else OK for t in range(len(sums))]
    assert one_batch[0] is False and one_batch[1] == one[0] and one_batch[2] is not None
    for chunk in (7, 2):                                                               # passes of at most 7 (2) entries and 7 (2) sums
        hooks(nat, chunk=chunk, short_max=3, piece=4)
        assert nat.tally_each(files, ss, en, claims, want_points=True) == one
        assert nat.tally_batch(files, ss, en, claims, SEED, want_status=True, want_point=True) == one_batch
        with _Dev(nat, files, ss, en, claims) as dev:
            assert nat.tally_each_device(*dev.args(), want_points=True) == one
