"""bppp_rp_excess_halfagg* and bppp_rp_excess_halfagg_verify*: the signatures of a job as their R rows and ONE scalar, checked as one MSM a pass.

The reference side is never the library under test: rangeproof.excess_halfagg_host restates the aggregate on hashlib and Python integers, and
rangeproof.excess_halfagg_verify_host the verdicts and the equation's left side over the oracle backend (tests/rp_backends.py).  The signatures come
from bppp_rp_excess_sign, which has its own tests.  One job of 2 T + 1 = 513 keys per handle is signed once and shared; every case is a prefix of it.
T = 256 is the tile of the hash tree's kernel: T - 1, T, T + 1 are one short, one full and two workgroups of the first launch, 2 T + 1 three."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from rp_backends import OracleBackend
from test_gpu_commit_open import _case, _native, _no_point_x

pytestmark = pytest.mark.gpu

N = O.N
AUX = hashlib.sha256(b"halfagg aux").digest()
OK, MISMATCH, NOT_CANONICAL, BAD_R, BAD_KEY = 0, 1, 3, 4, 6
NAMES = ["rec_test", "bin_test"]
T = 256
SIZES = [1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
AGG = RP.EXCESS_AGG_BYTES
_JOBS = {}


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
def flat_chunk():
    """bppp_test_rp_set_flat_chunk on one handle, restored afterwards"""
    tl, touched = capi.load_test_library(), []

    def set_(nat, items):
        touched.append(nat)
        assert tl.bppp_test_rp_set_flat_chunk(nat.h, items) == 0
    yield set_
    for nat in touched:
        assert tl.bppp_test_rp_set_flat_chunk(nat.h, 0) == 0


class _Dev:
    """arrays of one call in HBM, freed on exit"""

    def __init__(self, gpu, **arrays):
        self.gpu = gpu
        self.d = {k: gpu.to_device(v) for k, v in arrays.items()}

    def __enter__(self):
        return self.d

    def __exit__(self, *exc):
        for p in self.d.values():
            self.gpu.free(p)


def _bytes(rows):
    return np.frombuffer(b"".join(rows) or b"\0", dtype=np.uint8)


def _job(nat, name, salt=b"", n=2 * T + 1):
    """(keys, msgs, sigs) of n valid kernels, signed on the device once per (handle, salt)"""
    if (name, salt) not in _JOBS:
        rng = random.Random(name.encode() + salt)
        es = [rng.randrange(1, N) for _ in range(n)]
        msgs = [hashlib.sha256(b"halfagg msg %d " % t + salt).digest() for t in range(n)]
        _JOBS[(name, salt)] = (nat.excess_keys(es), msgs, nat.excess_sign(es, msgs, AUX))
    return tuple(list(a) for a in _JOBS[(name, salt)])


def _s_of(b32):
    return sum(int.from_bytes(b32[8 * i:8 * i + 8], "big") << (64 * i) for i in range(4))


def _with_s(agg, s):
    return agg[:-32] + RP._put(s)


def _agg_both(nat, keys, msgs, sigs):
    """the host call's (aggregate, statuses), after the _device variant has given the same into a buffer that was not zero"""
    host = nat.excess_halfagg(keys, msgs, sigs, want_status=True)
    n = len(keys)
    with _Dev(nat.gpu, k=_bytes(keys), m=_bytes(msgs), g=_bytes(sigs), a=np.full(AGG(n), 0xA5, dtype=np.uint8)) as d:
        st = nat.excess_halfagg_device(n, d["k"], d["m"], d["g"], d["a"], want_status=True)
        assert (nat.gpu.download(d["a"], (AGG(n),), np.uint8).tobytes(), st) == host
    return host


def _verify_both(nat, keys, msgs, agg):
    host = nat.excess_halfagg_verify(keys, msgs, agg, want_status=True, want_point=True)
    with _Dev(nat.gpu, k=_bytes(keys), m=_bytes(msgs), a=np.frombuffer(agg, dtype=np.uint8)) as d:
        assert nat.excess_halfagg_verify_device(len(keys), d["k"], d["m"], d["a"], want_status=True, want_point=True) == host
    return host


# ----------------------------------------------------------------------------- 1. the aggregate's bytes, and that it is accepted
@pytest.mark.parametrize("name", NAMES)
def test_aggregate_bytes_and_acceptance(gpu, handles, name):
    nat = handles(name)
    keys, msgs, sigs = _job(nat, name)
    for n in SIZES:
        want = RP.excess_halfagg_host(b"", keys[:n], msgs[:n], sigs[:n])
        assert len(want) == AGG(n) and want != bytes(AGG(n))
        assert _agg_both(nat, keys[:n], msgs[:n], sigs[:n]) == (want, [OK] * n), n
        assert _verify_both(nat, keys[:n], msgs[:n], want) == (True, [OK] * n, None), n
        assert nat.excess_halfagg(keys[:n], msgs[:n], sigs[:n]) == want and nat.excess_halfagg_verify(keys[:n], msgs[:n], want) is True
    # the aggregate of a prefix is not a prefix of the aggregate: every coefficient hangs on n and on the root
    assert RP.excess_halfagg_host(b"", keys[:3], msgs[:3], sigs[:3])[-32:] != RP.excess_halfagg_host(b"", keys[:2], msgs[:2], sigs[:2])[-32:]


# ----------------------------------------------------------------------------- 2. several passes over the workspace
@pytest.mark.parametrize("name", NAMES)
def test_passes_of_two_keys(gpu, oracle_lib, handles, flat_chunk, name):
    """a flat chunk of 8 is two keys a pass: n = 7 takes four passes, the last of one key; s_agg B is counted once for the job"""
    nat, st, be = handles(name), _case(oracle_lib, name)[0], OracleBackend(oracle_lib)
    keys, msgs, sigs = _job(nat, name)
    keys, msgs, sigs = keys[:7], msgs[:7], sigs[:7]
    agg = RP.excess_halfagg_host(b"", keys, msgs, sigs)
    bent = _with_s(agg, (_s_of(agg[-32:]) + 1) % N)
    one = (_agg_both(nat, keys, msgs, sigs), _verify_both(nat, keys, msgs, agg), _verify_both(nat, keys, msgs, bent))
    flat_chunk(nat, 8)
    assert (_agg_both(nat, keys, msgs, sigs), _verify_both(nat, keys, msgs, agg), _verify_both(nat, keys, msgs, bent)) == one
    _, _, B = RP._excess_bases(st)
    assert one == ((agg, [OK] * 7), (True, [OK] * 7, None), (False, [MISMATCH] * 7, B))      # s_agg + 1 leaves exactly one B: not one per pass
    assert one[2] == RP.excess_halfagg_verify_host(be, st, keys, msgs, bent, b"")


# ----------------------------------------------------------------------------- 3. verdicts and the equation's left side against the oracle
def _changes(ec, n, keys, msgs, agg, other):
    """every single-place change of a job of n keys (other: a valid key of another kernel): name -> (keys, msgs, agg, the status the changed key must
    get, that of the others)"""
    bx, last = RP._put(_no_point_x(ec)), n - 1
    row = lambda r: agg[:33 * last] + r + agg[33 * n:]
    key = lambda k: keys[:last] + [k]
    s = _s_of(agg[-32:])
    return {
        "key sign flipped": (key(keys[last][:32] + bytes([keys[last][32] ^ 1])), msgs, agg, MISMATCH, MISMATCH),
        "another key": (key(other), msgs, agg, MISMATCH, MISMATCH),
        "key sign byte 2": (key(keys[last][:32] + b"\x02"), msgs, agg, BAD_KEY, MISMATCH),
        "key x without a point": (key(bx + keys[last][32:]), msgs, agg, BAD_KEY, MISMATCH),
        "R sign flipped": (keys, msgs, row(agg[33 * last:33 * last + 32] + bytes([agg[33 * last + 32] ^ 1])), MISMATCH, MISMATCH),
        "R sign byte 2": (keys, msgs, row(agg[33 * last:33 * last + 32] + b"\x02"), BAD_R, MISMATCH),
        "R x without a point": (keys, msgs, row(bx + agg[33 * last + 32:33 * n]), BAD_R, MISMATCH),
        "message": (keys, msgs[:last] + [msgs[last][:-1] + bytes([msgs[last][-1] ^ 1])], agg, MISMATCH, MISMATCH),
        "s_agg + 1": (keys, msgs, _with_s(agg, (s + 1) % N), MISMATCH, MISMATCH),
        "s_agg = n": (keys, msgs, _with_s(agg, N), NOT_CANONICAL, NOT_CANONICAL),
        "s_agg = 2^256 - 1": (keys, msgs, _with_s(agg, 2**256 - 1), NOT_CANONICAL, NOT_CANONICAL),
        "bad key and s_agg = n": (key(keys[last][:32] + b"\x07"), msgs, _with_s(agg, N), BAD_KEY, NOT_CANONICAL),
    }


@pytest.mark.parametrize("name", NAMES)
def test_verdicts_and_the_combined_point(gpu, oracle_lib, handles, name):
    nat, st, be, ec = handles(name), _case(oracle_lib, name)[0], OracleBackend(oracle_lib), oracle_lib
    allk, allm, alls = _job(nat, name)
    for n in (1, 2, 5):
        keys, msgs, sigs = allk[:n], allm[:n], alls[:n]
        agg = nat.excess_halfagg(keys, msgs, sigs)
        assert _verify_both(nat, keys, msgs, agg) == (True, [OK] * n, None) == RP.excess_halfagg_verify_host(be, st, keys, msgs, agg, b"")
        for what, (k, m, a, changed, others) in _changes(ec, n, keys, msgs, agg, allk[n]).items():
            got = _verify_both(nat, k, m, a)
            assert got[0] is False and got[1] == [others] * (n - 1) + [changed], (n, what)
            assert got == RP.excess_halfagg_verify_host(be, st, k, m, a, b""), (n, what)        # the left side too: the oracle's evaluation
            assert nat.excess_halfagg_verify(k, m, a) is False
            assert got[2] is not None or (n, what) == (1, "bad key and s_agg = n"), (n, what)   # no term is left there: the identity, and rejected
    # a valid verdict never survives two rows of the job being swapped: the triples whole, or the keys and messages under the old rows
    keys, msgs, sigs = allk[:5], allm[:5], alls[:5]
    agg = nat.excess_halfagg(keys, msgs, sigs)
    sw = lambda xs: [xs[0], xs[3], xs[2], xs[1], xs[4]]
    rows = sw([agg[33 * i:33 * i + 33] for i in range(5)])
    assert _verify_both(nat, sw(keys), sw(msgs), b"".join(rows) + agg[-32:])[:2] == (False, [MISMATCH] * 5)
    assert _verify_both(nat, sw(keys), sw(msgs), agg)[:2] == (False, [MISMATCH] * 5)
    assert nat.excess_halfagg(sw(keys), sw(msgs), sw(sigs))[-32:] != agg[-32:]          # the swapped job has an aggregate of its own, which is accepted
    assert nat.excess_halfagg_verify(sw(keys), sw(msgs), nat.excess_halfagg(sw(keys), sw(msgs), sw(sigs))) is True


# ----------------------------------------------------------------------------- 4. the cancelling pair: the equation stays out of the aggregator
@pytest.mark.parametrize("name", NAMES)
def test_a_cancelling_pair(gpu, oracle_lib, handles, name):
    nat, st, be = handles(name), _case(oracle_lib, name)[0], OracleBackend(oracle_lib)
    keys, msgs, sigs = (a[:4] for a in _job(nat, name))
    s = [_s_of(g[33:]) for g in sigs]
    bent = [sigs[0], sigs[1][:33] + RP._put((s[1] + 1) % N), sigs[2], sigs[3][:33] + RP._put((s[3] - 1) % N)]
    assert sum(_s_of(g[33:]) for g in bent) % N == sum(s) % N                           # the plain sum has not moved
    assert nat.excess_verify_keys_each(keys, msgs, bent) == [OK, MISMATCH, OK, MISMATCH]
    agg, status = _agg_both(nat, keys, msgs, bent)
    assert status == [OK] * 4 and agg == RP.excess_halfagg_host(b"", keys, msgs, bent) and agg != bytes(AGG(4))
    got = _verify_both(nat, keys, msgs, agg)
    assert got[:2] == (False, [MISMATCH] * 4) and got[2] is not None and got == RP.excess_halfagg_verify_host(be, st, keys, msgs, agg, b"")


# ----------------------------------------------------------------------------- 5. the aggregator's refusals
@pytest.mark.parametrize("name", NAMES)
def test_aggregator_refusals(gpu, oracle_lib, handles, name):
    nat, ec = handles(name), oracle_lib
    keys, msgs, sigs = (a[:70] for a in _job(nat, name))
    bx = RP._put(_no_point_x(ec))
    cases = {"s = n": (3, keys[3], sigs[3][:33] + RP._put(N), NOT_CANONICAL, r"key 3: s is not canonical"),
             "key sign byte 2": (68, keys[68][:32] + b"\x02", sigs[68], BAD_KEY, r"key 68: the key's sign byte"),
             "key x without a point": (0, bx + keys[0][32:], sigs[0], BAD_KEY, r"key 0: the key's sign byte"),
             "R sign byte 3": (65, keys[65], sigs[65][:32] + b"\x03" + sigs[65][33:], BAD_R, r"key 65: the sign byte of R"),
             "R x without a point": (64, keys[64], bx + sigs[64][32:], BAD_R, r"key 64: the sign byte of R"),
             "bad key, bad R and s = n": (9, keys[9][:32] + b"\x02", bx + b"\x05" + RP._put(N), BAD_KEY, r"key 9: the key's sign byte"),
             "bad R and s = n": (9, keys[9], bx + b"\x00" + RP._put(N), NOT_CANONICAL, r"key 9: s is not canonical")}
    for what, (t, k, g, verdict, text) in cases.items():
        ks, gs = keys[:t] + [k] + keys[t + 1:], sigs[:t] + [g] + sigs[t + 1:]
        assert _agg_both(nat, ks, msgs, gs) == (bytes(AGG(70)), [verdict if i == t else OK for i in range(70)]), what
        assert RP.excess_halfagg_host(b"", ks, msgs, gs) == bytes(AGG(70))
        with pytest.raises(capi.BpppError, match=r"rp_excess_halfagg: " + text):
            nat.excess_halfagg(ks, msgs, gs)
    # two refusals: the error names the lowest; the host call still hands the zero bytes down
    ks, gs = [keys[0]] + [keys[1][:32] + b"\x02"] + keys[2:], sigs[:40] + [sigs[40][:33] + RP._put(N)] + sigs[41:]
    out = np.full(AGG(70), 0xA5, dtype=np.uint8)
    args = [C.c_void_p(a.ctypes.data) for a in (_bytes(ks), _bytes(msgs), _bytes(gs), out)]
    assert gpu.lib.bppp_rp_excess_halfagg(nat.h, 70, *args, None) == -1 and gpu.lib.bppp_last_error(gpu.h).startswith(b"rp_excess_halfagg: key 1: ")
    assert out.tobytes() == bytes(AGG(70))


# ----------------------------------------------------------------------------- 6. nothing rests on what an earlier call left in the workspaces
def _poison(byte, gpu, nat):
    tlib, n, total = capi.load_test_library(), C.c_uint64(0), 0
    assert tlib.bppp_test_ctx_poison(gpu.h, byte, C.byref(n)) == 0
    total += n.value
    assert tlib.bppp_test_rp_poison(nat.h, byte, C.byref(n)) == 0
    return total + n.value


@pytest.mark.parametrize("name", NAMES)
def test_after_poisoned_workspaces(gpu, oracle_lib, handles, flat_chunk, name):
    """a larger job on other inputs warms the buffers, poison, then the measured call: zero first, then 0xA5; one pass and passes of two keys.  The
    rejected aggregate is s_agg + 5, whose left side is 5 B by the oracle."""
    nat, st, ec = handles(name), _case(oracle_lib, name)[0], oracle_lib
    wk, wm, wg = _job(nat, name, b"warm", 300)
    wagg = RP.excess_halfagg_host(b"", wk, wm, wg)
    keys, msgs, sigs = _job(nat, name)
    five_b = ec.mul(5, RP._excess_bases(st)[2])
    for chunk, n in ((0, 261), (8, 7)):
        if chunk:
            flat_chunk(nat, chunk)
        k, m, g = keys[:n], msgs[:n], sigs[:n]
        agg = RP.excess_halfagg_host(b"", k, m, g)
        bad = _with_s(agg, (_s_of(agg[-32:]) + 5) % N)
        calls = ((lambda: _agg_both(nat, k, m, g), (agg, [OK] * n)), (lambda: _verify_both(nat, k, m, agg), (True, [OK] * n, None)),
                 (lambda: _verify_both(nat, k, m, bad), (False, [MISMATCH] * n, five_b)))
        for byte in (0x00, 0xA5):
            for call, expect in calls:
                assert nat.excess_halfagg(wk, wm, wg) == wagg and nat.excess_halfagg_verify(wk, wm, wagg) is True
                assert _poison(byte, gpu, nat) > 0
                assert call() == expect, (chunk, byte)


# ----------------------------------------------------------------------------- 7. arguments
def test_arguments(gpu, oracle_lib, handles):
    nat = handles("rec_test")
    lib, err = gpu.lib, lambda: gpu.lib.bppp_last_error(gpu.h)
    keys, msgs, sigs = (a[:2] for a in _job(nat, "rec_test"))
    agg = nat.excess_halfagg(keys, msgs, sigs)
    # no key: accepted, nothing is looked at, the aggregator writes nothing
    assert nat.excess_halfagg([], [], []) == b"" and nat.excess_halfagg([], [], [], want_status=True) == (b"", [])
    assert nat.excess_halfagg_verify([], [], b"") is True and nat.excess_halfagg_verify([], [], b"", want_status=True, want_point=True) == (True, [], None)
    acc, out = C.c_int(7), np.full(AGG(2), 0xA5, dtype=np.uint8)
    assert lib.bppp_rp_excess_halfagg(nat.h, 0, None, None, None, C.c_void_p(out.ctypes.data), None) == 0 and out.tobytes() == b"\xa5" * AGG(2)
    assert lib.bppp_rp_excess_halfagg_device(nat.h, 0, None, None, None, None, None) == 0
    assert lib.bppp_rp_excess_halfagg_verify(nat.h, 0, None, None, None, C.byref(acc), None, None) == 0 and acc.value == 1
    acc.value = 7
    assert lib.bppp_rp_excess_halfagg_verify_device(nat.h, 0, None, None, None, C.byref(acc), None, None) == 0 and acc.value == 1
    # null buffers, a missing accept and sizes at 2^31
    p = [C.c_void_p(a.ctypes.data) for a in (_bytes(keys), _bytes(msgs), _bytes(sigs), np.frombuffer(agg, dtype=np.uint8))]
    for hole in range(4):
        a = [None if i == hole else p[i] for i in range(3)] + [None if hole == 3 else C.c_void_p(out.ctypes.data)]
        assert lib.bppp_rp_excess_halfagg(nat.h, 2, *a, None) == -1 and b"rp_excess_halfagg: null input" in err(), hole
    for hole in range(3):
        a = [None if i == hole else (p[i] if i < 2 else p[3]) for i in range(3)]
        assert lib.bppp_rp_excess_halfagg_verify(nat.h, 2, *a, C.byref(acc), None, None) == -1 and b"rp_excess_halfagg_verify: null input" in err(), hole
    assert lib.bppp_rp_excess_halfagg_verify(nat.h, 2, p[0], p[1], p[3], None, None, None) == -1
    for big in (2**31, 2**40):
        assert lib.bppp_rp_excess_halfagg(nat.h, big, p[0], p[1], p[2], C.c_void_p(out.ctypes.data), None) == -1 and b"nkeys must be below 2^31" in err()
        assert lib.bppp_rp_excess_halfagg_device(nat.h, big, p[0], p[1], p[2], p[3], None) == -1 and b"nkeys must be below 2^31" in err()
        assert lib.bppp_rp_excess_halfagg_verify(nat.h, big, p[0], p[1], p[3], C.byref(acc), None, None) == -1 and b"nkeys must be below 2^31" in err()
        assert lib.bppp_rp_excess_halfagg_verify_device(nat.h, big, p[0], p[1], p[3], C.byref(acc), None, None) == -1 and b"nkeys must be below 2^31" in err()
    assert out.tobytes() == b"\xa5" * AGG(2)                                        # no output buffer is written on an error
    assert nat.excess_halfagg_verify(keys, msgs, agg) is True
