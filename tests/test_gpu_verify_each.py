"""bppp_rp_verify_each*: every range proof of a batch decided on its own, without weights — E_b = MSM(T_b) over the term list verifyWith
builds for proof b alone, valid iff E_b is the identity — and BPPP_RP_OPT_CULPRITS = 1, which resolves a rejected batch with one such pass
instead of bisection.  Statuses must equal each proof's own verify_batch(batch = 1) verdict and the bisection's; the points must add up,
under verify_batch's weights rho (restated here from include/bppp.h), to its combined point."""
import ctypes as C
import hashlib
import json
import os
import random
import struct

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import encoding as E
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import BpppError, array_to_point, load_test_library, points_to_array
from test_rangeproof import EXAMPLES

pytestmark = pytest.mark.gpu

SEED = hashlib.sha256(b"verify each seed").digest()
P = 2**256 - 2**32 - 977
VALID, INVALID, MALFORMED = 0, 1, 2


# ----------------------------------------------------------------------------- setups and proofs (the library's own prover)
def _nl_setup(gpu, typed):
    pts = O.hash_points(b"verify each", 120)
    rds = [RP.make_range_data(4, 0, 256, True, True, False), RP.make_range_data(4, 10, 266, True, True, False),
           RP.make_range_data(16, 0, 2**64, False, True, False), RP.make_range_data(3, 0, 100, False, True, False)]
    pub = [(False, 7, 500)] if typed else []
    return RP.NativeRangeProofs(gpu, RP.setup(RP.GpuBackend(gpu), pts, typed, pub, rds, "NL"))


def _nl_inputs(typed, n, seed):
    rnd = random.Random(seed)
    if typed:
        return [[(v, 7, rnd.randrange(O.N)) for v in (200, 20, 250, 30)] for _ in range(n)]
    return [[(rnd.randrange(256), 0, rnd.randrange(O.N)), (10 + rnd.randrange(256), 0, rnd.randrange(O.N)), (rnd.randrange(2**64), 0, rnd.randrange(O.N)),
             (rnd.randrange(100), 0, rnd.randrange(O.N))] for _ in range(n)]


def _example(gpu, name):
    schema = json.load(open(os.path.join(EXAMPLES, name, "schema.json")))
    if schema.get("binary", False):
        return BRP.NativeBinaryRangeProofs(gpu, BRP.setup_from_schema(RP.GpuBackend(gpu), schema)), True
    return RP.NativeRangeProofs(gpu, RP.setup_from_schema(RP.GpuBackend(gpu), schema)), False


def _example_inputs(name, binary, n, seed):
    wit = json.load(open(os.path.join(EXAMPLES, name, "witness.json")))
    out = []
    for j in range(n):
        rows = RP.inputs_from_witness(wit, b"each %s %d %d" % (name.encode(), seed, j))
        out.append([(v, bl) for v, _, bl in rows] if binary else rows)
    return out


def _make(gpu, kind):
    if kind in ("nl", "typed"):
        typed = kind == "typed"
        return _nl_setup(gpu, typed), (lambda n, seed: _nl_inputs(typed, n, seed))
    nat, binary = _example(gpu, kind)
    return nat, (lambda n, seed: _example_inputs(kind, binary, n, seed))


def _prove(nat, inputs_fn, n, seed=1):
    files = nat.prove_batch(inputs_fn(n, seed), [b"each random %04d %06d" % (seed, j) for j in range(n)])
    return [c for c, _ in files], [p for _, p in files]


@pytest.fixture(scope="module")
def handles(gpu):
    hs = {}
    yield hs
    for nat, _ in hs.values():
        nat.close()


def _handle(gpu, handles, kind):
    if kind not in handles:
        handles[kind] = _make(gpu, kind)
    return handles[kind]


# ----------------------------------------------------------------------------- tampering
def _non_liftable_x():
    x = 5
    while pow((x ** 3 + 7) % P, (P - 1) // 2, P) == 1:
        x += 1
    return x


def _tamper(nat, cf, pf, b, how):
    """proof b of the batch, changed as `how` says; returns the expected status"""
    s = nat.shape
    if how == "sign":                   # the sign bit of the proof's first point: the negated point still decodes
        p = bytearray(pf[b]); p[32 * (s["final_norm"] + s["final_lin"])] ^= 1; pf[b] = bytes(p)
        return INVALID
    if how == "witness":                # a final-witness scalar changed
        p = bytearray(pf[b]); p[31] ^= 4; pf[b] = bytes(p)
        return INVALID
    if how == "malformed":              # an input commitment whose x has no curve point
        c = bytearray(cf[b]); sb = (s["nranges"] + 7) // 8
        c[sb:sb + 32] = E.put_field(_non_liftable_x()); cf[b] = bytes(c)
        return MALFORMED
    if how == "swap":                   # the commitments of another proof
        cf[b] = cf[(b + 1) % len(cf)]
        return INVALID
    raise ValueError(how)


KINDS = ["sign", "witness", "malformed", "swap"]


def _tampered_batch(nat, inputs_fn, n, bad, seed=1):
    cf, pf = _prove(nat, inputs_fn, n, seed)
    want = [VALID] * n
    for j, b in enumerate(bad):             # (callers keep the proof after a swapped one untouched)
        want[b] = _tamper(nat, cf, pf, b, KINDS[j % len(KINDS)])
    return cf, pf, want


# ----------------------------------------------------------------------------- the weights of verify_batch, restated (include/bppp.h)
def _fr_be(raw):
    """Binary (Prime p) get of 32 bytes: four big-endian 64-bit words, least significant first; reduced"""
    return sum(int.from_bytes(raw[8 * i:8 * i + 8], "big") << (64 * i) for i in range(4)) % O.N


def _rho(nat, seed, idx, t, e_last, pfile):
    s = nat.shape
    wit = [_fr_be(pfile[32 * i:32 * i + 32]) for i in range(s["final_norm"] + s["final_lin"])]
    msg = seed + struct.pack("<Q", idx) + t.to_bytes(32, "little") + (e_last.to_bytes(32, "little") if s["rounds"] else b"")
    msg += b"".join(w.to_bytes(32, "little") for w in wit)
    return _fr_be(hashlib.sha256(msg).digest()) or 1


def _batch_full(gpu, nat, cf, pf, seed=SEED):
    """bppp_rp_verify_batch with everything: (accept, statuses, challenges, combined point)"""
    B = len(pf)
    acc, out = C.c_int(0), np.zeros(8, dtype=np.uint64)
    st = np.zeros(max(B, 1), dtype=np.uint32)
    nch = nat.shape["challenges_per_proof"]
    ch = np.zeros((max(B, 1) * nch, 4), dtype=np.uint64)
    cb, pb = np.frombuffer(b"".join(cf), dtype=np.uint8), np.frombuffer(b"".join(pf), dtype=np.uint8)
    sd = np.frombuffer(seed, dtype=np.uint8)
    rc = gpu.lib.bppp_rp_verify_batch(nat.h, B, C.c_void_p(cb.ctypes.data), C.c_void_p(pb.ctypes.data), C.c_void_p(sd.ctypes.data), C.byref(acc),
                                      C.c_void_p(st.ctypes.data), C.c_void_p(ch.ctypes.data), C.c_void_p(out.ctypes.data))
    gpu._check(rc, "bppp_rp_verify_batch")
    from bulletproofspp_amd.capi import array_to_scalars
    flat = array_to_scalars(ch)
    chs = [flat[b * nch:(b + 1) * nch] for b in range(B)]
    return bool(acc.value), [int(v) for v in st[:B]], chs, array_to_point(out)


def _check_points(gpu, nat, cf, pf, status, pts):
    """sum_b rho_b E_b equals verify_batch's combined point (no malformed proof in the batch); valid proofs have E_b = infinity"""
    assert MALFORMED not in status
    for s_, e in zip(status, pts):
        assert (s_ == VALID) == (e is None)
    _, _, chs, comb = _batch_full(gpu, nat, cf, pf)
    lead = nat.shape["challenges_per_proof"] - nat.shape["rounds"]
    terms = []
    for b, e in enumerate(pts):
        if e is None:
            continue
        t = chs[b][lead - 1]                        # t: the last range-proof challenge (7 typed reciprocal, 4 binary)
        e_last = chs[b][lead] if nat.shape["rounds"] else 0
        terms.append((_rho(nat, SEED, b, t, e_last, pf[b]), e))
    want = O.CEC().inner_product(terms) if terms else None
    assert comb == want


def _counts(nat):
    a, b = C.c_uint64(0), C.c_uint64(0)
    assert load_test_library().bppp_test_rp_last_verify_counts(nat.h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _up(gpu, bs):
    raw = b"".join(bs) or b"\0"
    return gpu.to_device(np.frombuffer(raw + b"\0" * (-len(raw) % 8), dtype=np.uint8).view(np.uint64))


# ----------------------------------------------------------------------------- statuses and points
SETUPS = ["nl", "typed", "64bit", "bin_test", "64by64"]


@pytest.mark.parametrize("kind", SETUPS)
def test_statuses_match_single_and_bisection(gpu, handles, kind):
    nat, inputs_fn = _handle(gpu, handles, kind)
    n = 11
    cf, pf, want = _tampered_batch(nat, inputs_fn, n, [1, 4, 6, 9])
    got = nat.verify_each(cf, pf)
    assert got == want
    singles = [nat.verify_batch([c], [p], SEED, want_status=True)[1][0] for c, p in zip(cf, pf)]
    assert got == singles
    ok, bis, _ = nat.verify_batch(cf, pf, SEED, want_status=True)
    assert not ok and got == bis
    assert _counts(nat)[1] == 0                                     # bisection by default
    # the device entry point on the same files
    dc, dp = _up(gpu, cf), _up(gpu, pf)
    try:
        st2, pts2 = nat.verify_each_device(n, dc, dp, want_points=True)
    finally:
        gpu.free(dc); gpu.free(dp)
    st1, pts1 = nat.verify_each(cf, pf, want_points=True)
    assert st1 == st2 == got and pts1 == pts2
    assert all(pts1[b] is None for b in range(n) if got[b] != INVALID)
    assert all(pts1[b] is not None for b in range(n) if got[b] == INVALID)
    assert _counts(nat) == (0, 1)


@pytest.mark.parametrize("kind", SETUPS)
def test_points_add_up_to_the_combined_point(gpu, handles, kind):
    nat, inputs_fn = _handle(gpu, handles, kind)
    n = 9
    cf, pf = _prove(nat, inputs_fn, n, seed=2)
    _tamper(nat, cf, pf, 2, "sign"); _tamper(nat, cf, pf, 5, "witness"); _tamper(nat, cf, pf, 7, "swap")
    status, pts = nat.verify_each(cf, pf, want_points=True)
    assert status == [VALID, VALID, INVALID, VALID, VALID, INVALID, VALID, INVALID, VALID]
    _check_points(gpu, nat, cf, pf, status, pts)


def test_edges(gpu, handles):
    nat, inputs_fn = _handle(gpu, handles, "nl")
    assert nat.verify_each([], []) == []
    assert nat.verify_each([], [], want_points=True) == ([], [])
    cf, pf = _prove(nat, inputs_fn, 70, seed=3)
    # all valid, batch 1, a batch that is not a multiple of 64
    assert nat.verify_each(cf[:1], pf[:1], want_points=True) == ([VALID], [None])
    assert nat.verify_each(cf, pf) == [VALID] * 70
    # all invalid
    bad_pf = list(pf[:13])
    for b in range(13):
        _tamper(nat, cf, bad_pf, b, "witness")
    st, pts = nat.verify_each(cf[:13], bad_pf, want_points=True)
    assert st == [INVALID] * 13
    _check_points(gpu, nat, cf[:13], bad_pf, st, pts)
    # a file of the wrong length: the whole batch MALFORMED without a library call, as verify_batch
    assert nat.verify_each(cf[:3], pf[:2] + [pf[2][:-1]]) == [MALFORMED] * 3
    assert nat.verify_batch(cf[:3], pf[:2] + [pf[2][:-1]], SEED, want_status=True)[1] == [MALFORMED] * 3


def test_chunks_and_comb_table(gpu):
    """the same statuses and points across chunk boundaries (the last chunk padded) and with or without the handle's comb table"""
    prover = _nl_setup(gpu, False)
    plain = _nl_setup(gpu, False)                  # never proves: no comb table, the registered basis serves the fixed-base part
    try:
        prover.set_option("comb_min", 8)
        prover.set_option("comb_bits", 8)          # a small table, quick to build
        cf, pf = _prove(prover, lambda n, s: _nl_inputs(False, n, s), 45, seed=4)      # >= comb_min: the prover built its table
        want = [VALID] * 45
        for j, b in enumerate([0, 9, 17, 30, 44]):
            want[b] = _tamper(prover, cf, pf, b, ["sign", "witness", "swap", "sign", "witness"][j])
        ref = plain.verify_each(cf, pf, want_points=True)
        assert ref[0] == want
        assert prover.verify_each(cf, pf, want_points=True) == ref
        tl = load_test_library()
        for nat in (plain, prover):
            assert tl.bppp_test_rp_set_each_chunk(nat.h, 8) == 0      # 45 = 5 x 8 + 5: six chunks, the last one padded
            assert nat.verify_each(cf, pf, want_points=True) == ref
            assert tl.bppp_test_rp_set_each_chunk(nat.h, 16) == 0
            assert nat.verify_each(cf, pf, want_points=True) == ref
            assert tl.bppp_test_rp_set_each_chunk(nat.h, 0) == 0
        _check_points(gpu, plain, cf, pf, ref[0], ref[1])
    finally:
        prover.close(); plain.close()


def test_argument_errors(gpu, handles):
    nat, inputs_fn = _handle(gpu, handles, "nl")
    cf, pf = _prove(nat, inputs_fn, 2, seed=5)
    st = np.zeros(2, dtype=np.uint32)
    cb = np.frombuffer(b"".join(cf), dtype=np.uint8)
    vpst = C.c_void_p(st.ctypes.data)
    lib = gpu.lib
    assert lib.bppp_rp_verify_each(None, 2, C.c_void_p(cb.ctypes.data), C.c_void_p(cb.ctypes.data), vpst, None) != 0
    assert lib.bppp_rp_verify_each(nat.h, 2, None, None, vpst, None) != 0                 # null files, non-empty batch
    assert lib.bppp_rp_verify_each_device(nat.h, 2, None, None, vpst, None) != 0
    assert lib.bppp_rp_verify_each(nat.h, 2, C.c_void_p(cb.ctypes.data), C.c_void_p(cb.ctypes.data), None, None) != 0    # no status array
    assert lib.bppp_rp_verify_each(nat.h, 0, None, None, vpst, None) == 0                  # empty batch
    assert lib.bppp_rp_verify_each_device(nat.h, 0, None, None, vpst, None) == 0
    with pytest.raises(BpppError):
        nat.set_option("culprits", 2)
    # the handle still verifies after the refusals
    assert nat.verify_each(cf, pf) == [VALID, VALID]


# ----------------------------------------------------------------------------- BPPP_RP_OPT_CULPRITS
@pytest.mark.parametrize("kind", ["nl", "bin_test", "64bit"])
def test_culprits_option(gpu, handles, kind):
    nat, inputs_fn = _handle(gpu, handles, kind)
    cf, pf, want = _tampered_batch(nat, inputs_fn, 37, [3, 5, 20, 31, 36], seed=6)
    try:
        nat.set_option("culprits", 0)
        ok0, st0, _ = nat.verify_batch(cf, pf, SEED, want_status=True)
        n_comb0, n_each0 = _counts(nat)
        assert not ok0 and st0 == want and n_each0 == 0 and n_comb0 > 1         # the accept check, then bisection
        nat.set_option("culprits", 1)
        ok1, st1, _ = nat.verify_batch(cf, pf, SEED, want_status=True)
        assert (ok1, st1) == (ok0, st0)
        assert _counts(nat) == (1, 1)                                            # the accept check and one per-proof pass
        # an accepted batch costs nothing more
        good_c, good_p = _prove(nat, inputs_fn, 5, seed=7)
        assert nat.verify_batch(good_c, good_p, SEED, want_status=True)[:2] == (True, [VALID] * 5)
        assert _counts(nat) == (1, 0)
    finally:
        nat.set_option("culprits", 0)


def test_culprits_option_mixed(gpu, handles):
    a, fa = _handle(gpu, handles, "nl")
    b, fb = _handle(gpu, handles, "bin_test")
    c, fc = _handle(gpu, handles, "64bit")
    ca, pa, wa = _tampered_batch(a, fa, 9, [2, 7], seed=8)
    cb, pb = _prove(b, fb, 6, seed=8)                       # a valid group
    cc, pc, wc = _tampered_batch(c, fc, 7, [0, 4], seed=8)
    groups = [(a, ca, pa), (b, cb, pb), (c, cc, pc)]
    want = wa + [VALID] * 6 + wc
    try:
        for h in (a, b, c):
            h.set_option("culprits", 0)
        ok0, st0 = RP.verify_mixed(gpu, groups, SEED, want_status=True)
        assert not ok0 and st0 == want
        for h in (a, b, c):
            h.set_option("culprits", 1)
        assert RP.verify_mixed(gpu, groups, SEED, want_status=True) == (ok0, st0)
        assert _counts(a) == (1, 1) and _counts(b) == (1, 0) and _counts(c) == (1, 1)   # each group's own check; one pass per failing group
    finally:
        for h in (a, b, c):
            h.set_option("culprits", 0)


# ----------------------------------------------------------------------------- scale
def test_4096_64by64_one_percent_tampered(gpu, handles):
    nat, inputs_fn = _handle(gpu, handles, "64by64")
    nat.set_option("comb_bits", 12)                 # the 4096-proof batch below builds the prover's table: keep it small
    n = 4096
    cf, pf = _prove(nat, inputs_fn, n, seed=9)
    rnd = random.Random(4096)
    bad = sorted(rnd.sample(range(n), 41))
    want = [VALID] * n
    for j, b in enumerate(bad):
        want[b] = _tamper(nat, cf, pf, b, ["sign", "witness", "malformed"][j % 3])
    assert nat.verify_each(cf, pf) == want
    try:
        nat.set_option("culprits", 1)
        ok, st, _ = nat.verify_batch(cf, pf, SEED, want_status=True)
        assert not ok and st == want and _counts(nat) == (1, 1)
    finally:
        nat.set_option("culprits", 0)
