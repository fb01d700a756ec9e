"""bppp_rp_excess_keys*, bppp_rp_excess_verify_keys_each*, bppp_rp_excess_verify_keys_batch*, bppp_rp_excess_sums_each*, bppp_rp_excess_sums_batch*:
the excess stated as a 33-byte key — signatures checked with no pool, sums checked after cut-through.

The reference side is the host protocol code over the oracle backend (tests/rp_backends.py): rangeproof.excess_key33 / excess_verify_key_host /
excess_sums_host restate the calls over the oracle's group law, rangeproof.tally_sums the sums, rangeproof.excess_weight and tally_weight the batch
weights — never the library under test.  The pools are test_gpu_commit_open's 65 rows per setup, computed once and shared; every job is a few dozen
sums or keys."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from rp_backends import OracleBackend
from test_gpu_commit_open import _case, _native, _no_point_x, _set_x

pytestmark = pytest.mark.gpu

N, P = O.N, RP.FIELD_P
SEED = hashlib.sha256(b"excess keys seed").digest()
AUX = hashlib.sha256(b"excess keys aux").digest()
OK, MISMATCH, MALFORMED, NOT_CANONICAL, BAD_R, NO_KEY, BAD_KEY = 0, 1, 2, 3, 4, 5, 6
NAMES = ["32bit", "bin_test", "rec_test", "nine"]
SUB = RP.TALLY_SUBTRACT
SIG, KEY = RP.EXCESS_SIG_BYTES, RP.EXCESS_KEY_BYTES
SHAPES = [(0, 0), (0, 1), (1, 0), (1, 1), (3, 2), (2, 17), (17, 2), (40, 40)]       # (entries, keys) of a sum


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


class _Dev:
    """arrays of one call in HBM, freed on exit; None stays 0 (a NULL argument)"""

    def __init__(self, gpu, **arrays):
        self.gpu = gpu
        self.d = {k: (gpu.to_device(v) if v is not None else 0) for k, v in arrays.items()}

    def __enter__(self):
        return self.d

    def __exit__(self, *exc):
        for p in self.d.values():
            if p:
                self.gpu.free(p)


def _bytes(rows):
    return np.frombuffer(b"".join(rows) or b"\0", dtype=np.uint8)


def _pool(oracle_lib, name):
    st, inputs, triples, pts, files = _case(oracle_lib, name)
    return st, inputs, [t for row in triples for t in row], [p for row in pts for p in row], files


def _blind_base(st, name):
    return st.hs[0] if name == "bin_test" else st.hs[1]


def _csr(sums):
    sum_start, entries = [0], []
    for s in sums:
        entries += [RP.tally_entry(j, sub) for j, sub in s]
        sum_start.append(len(entries))
    return sum_start, entries


def _msgs(n, salt=b""):
    return [hashlib.sha256(b"excess keys msg %d " % t + salt).digest() for t in range(n)]


def _s_of(sig):
    return sum(int.from_bytes(sig[33 + 8 * i:41 + 8 * i], "big") << (64 * i) for i in range(4))


def _with_s(sig, s):
    return sig[:33] + RP._put(s)


def _scalars(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(1, N) for _ in range(n)]


MUTATIONS = ["s+1", "message", "key sign flipped", "another key", "s=n", "R sign 2", "R.x no point", "key sign 2", "key.x no point", "bad key and bad R and s=n",
             "bad R and s=n"]
EXPECT = {"s+1": MISMATCH, "message": MISMATCH, "key sign flipped": MISMATCH, "another key": MISMATCH, "s=n": NOT_CANONICAL, "R sign 2": BAD_R, "R.x no point": BAD_R,
          "key sign 2": BAD_KEY, "key.x no point": BAD_KEY, "bad key and bad R and s=n": BAD_KEY, "bad R and s=n": NOT_CANONICAL}


def _mutate(ec, keys, msgs, sigs, first=1, step=2):
    """one mutation at positions first, first + step, ...; returns where each went"""
    bx = RP._put(_no_point_x(ec))
    at = {m: first + step * i for i, m in enumerate(MUTATIONS)}
    f = {"s+1": lambda k, m, g: (k, m, _with_s(g, (_s_of(g) + 1) % N)),
         "message": lambda k, m, g: (k, m[:-1] + bytes([m[-1] ^ 1]), g),
         "key sign flipped": lambda k, m, g: (k[:32] + bytes([k[32] ^ 1]), m, g),
         "another key": lambda k, m, g: (keys[0], m, g),
         "s=n": lambda k, m, g: (k, m, _with_s(g, N)),
         "R sign 2": lambda k, m, g: (k, m, g[:32] + b"\x02" + g[33:]),
         "R.x no point": lambda k, m, g: (k, m, bx + g[32:]),
         "key sign 2": lambda k, m, g: (k[:32] + b"\x02", m, g),
         "key.x no point": lambda k, m, g: (bx + k[32:], m, g),
         "bad key and bad R and s=n": lambda k, m, g: (k[:32] + b"\x09", m, bx + b"\x00" + RP._put(N)),
         "bad R and s=n": lambda k, m, g: (k, m, g[:32] + b"\x03" + RP._put(N))}
    for name, t in at.items():
        keys[t], msgs[t], sigs[t] = f[name](keys[t], msgs[t], sigs[t])
    return at


# ----------------------------------------------------------------------------- 1. the builder's keys
@pytest.mark.parametrize("name", NAMES)
def test_builder_keys(gpu, oracle_lib, handles, name):
    st = _case(oracle_lib, name)[0]
    nat, ec, B = handles(name), oracle_lib, _blind_base(_case(oracle_lib, name)[0], name)
    es = _scalars(6, 11) + [1, 2, N - 1, 2**255, 2**128]
    want = [RP.excess_key33(ec.mul(e, B)) for e in es]
    assert nat.excess_keys(es, want_status=True) == (want, [0] * len(es))
    assert nat.excess_keys(es) == want
    assert nat.excess_sign(es, _msgs(len(es)), AUX, want_points=True)[2] == [RP.excess_lift33(k) for k in want]     # the signer's X is the key's point
    es2 = [es[0], 0, N, es[3], 2**256 - 1]
    want2 = ([want[0], bytes(KEY), bytes(KEY), want[3], bytes(KEY)], [0, capi.RP_EXCESS_ZERO, capi.RP_EXCESS_NOT_CANONICAL, 0, capi.RP_EXCESS_NOT_CANONICAL])
    assert nat.excess_keys(es2, want_status=True) == want2
    with pytest.raises(capi.BpppError, match=r"rp_excess_keys: sum 1: .*zero"):
        nat.excess_keys(es2)
    with pytest.raises(capi.BpppError, match=r"rp_excess_keys: sum 2: .*not canonical"):
        nat.excess_keys([es[0], es[1], N, 0])
    with _Dev(gpu, bl=capi.scalars_to_array(es2), ks=np.full(len(es2) * KEY, 0xA5, dtype=np.uint8)) as d:
        assert nat.excess_keys_device(len(es2), d["bl"], d["ks"], want_status=True) == want2[1]
        raw = gpu.download(d["ks"], (len(es2) * KEY,), np.uint8).tobytes()
        assert [raw[t * KEY:(t + 1) * KEY] for t in range(len(es2))] == want2[0]
    assert nat.excess_keys([]) == []
    assert gpu.lib.bppp_rp_excess_keys(nat.h, 1, None, None, None) == -1 and b"null input" in gpu.lib.bppp_last_error(gpu.h)


# ----------------------------------------------------------------------------- 2. existing signatures verify unchanged under the stated key
def _keys_each_both(nat, keys, msgs, sigs):
    host = nat.excess_verify_keys_each(keys, msgs, sigs)
    with _Dev(nat.gpu, k=_bytes(keys), m=_bytes(msgs), g=_bytes(sigs)) as d:
        assert nat.excess_verify_keys_each_device(len(keys), d["k"], d["m"], d["g"]) == host
    return host


@pytest.mark.parametrize("name", NAMES)
def test_existing_signatures_verify_unchanged(gpu, oracle_lib, handles, name):
    st = _case(oracle_lib, name)[0]
    nat, be, ec = handles(name), OracleBackend(oracle_lib), oracle_lib
    es, msgs = _scalars(65, 21), _msgs(65)
    sigs, keys = nat.excess_sign(es, msgs, AUX), nat.excess_keys(es)
    assert _keys_each_both(nat, keys, msgs, sigs) == [OK] * 65
    at = _mutate(ec, keys, msgs, sigs)
    want = [RP.excess_verify_key_host(be, st, k, m, g, b"") for k, m, g in zip(keys, msgs, sigs)]
    assert want == [next((EXPECT[m] for m, t in at.items() if t == i), OK) for i in range(65)]
    for n in (1, 15, 16, 17, 63, 64, 65):                                              # quad and block edges of 64-lane launches, four lanes a key
        assert _keys_each_both(nat, keys[:n], msgs[:n], sigs[:n]) == want[:n], n
    assert nat.excess_verify_keys_each([], [], []) == []


# ----------------------------------------------------------------------------- 3. the derived-key path and the stated-key path agree
def _lift(ec, b33):
    x = RP.decode_field(b33[:32], P)
    y = ec.lift_x(x)[1]
    return (x, y if (y > P - y) == bool(b33[32]) else P - y)


def _combined_keys(ec, B, seed, offset, keys, msgs, sigs, lo, hi):
    """sum over t in [lo, hi) of rho_t (s_t B - c_t X_t - R_t), by the oracle; every t has a verdict of the equation"""
    terms = []
    for t in range(lo, hi):
        X = _lift(ec, keys[t])
        rho = RP.excess_weight(seed, offset + t, sigs[t], X, msgs[t])
        c = RP.excess_challenge(b"", sigs[t][:33], X, msgs[t])
        terms += [(rho * _s_of(sigs[t]) % N, B), ((-rho * c) % N, X), ((-rho) % N, _lift(ec, sigs[t][:33]))]
    return ec.inner_product(terms)


@pytest.mark.parametrize("name", ["rec_test", "bin_test"])
def test_agrees_with_the_derived_key_path(gpu, oracle_lib, handles, name):
    st, inputs, triples, flat, files = _pool(oracle_lib, name)
    nat, ec, typed = handles(name), oracle_lib, name != "bin_test"
    rng = random.Random(31)
    sums = [[(rng.randrange(len(flat)), rng.random() < 0.4) for _ in range(n)] for n in [1, 2, 3, 5, 8, 1, 20, 4, 2, 7, 3, 6]]
    ss, en = _csr(sums)
    host_claims = RP.tally_claims_host(triples, ss, en)
    public = [(a, ty) if typed else (a,) for a, ty, _ in host_claims]
    msgs = _msgs(len(sums), b"derived")
    sigs = nat.excess_sign([e for _, _, e in host_claims], msgs, AUX)
    sigs[1] = _with_s(sigs[1], (_s_of(sigs[1]) + 1) % N)
    msgs[4] = msgs[4][::-1]
    pool_status, X = nat.excess_verify_each(files, ss, en, public, msgs, sigs, want_points=True)
    assert pool_status == [MISMATCH if t in (1, 4) else OK for t in range(len(sums))] and None not in X
    keys = [RP.excess_key33(x) for x in X]
    assert nat.excess_verify_keys_each(keys, msgs, sigs) == pool_status
    acc, status, point = nat.excess_verify_keys_batch(keys, msgs, sigs, SEED, want_status=True, want_point=True)
    assert not acc and status == pool_status and point == _combined_keys(ec, _blind_base(st, name), SEED, 0, keys, msgs, sigs, 0, len(sums)) and point is not None
    assert nat.excess_verify_batch(files, ss, en, public, msgs, sigs, SEED, want_point=True)[2] == point       # the same weights: one combined point on both paths
    sigs[2] = _with_s(sigs[2], N)
    sigs[6] = sigs[6][:32] + b"\x02" + sigs[6][33:]
    sigs[8] = RP._put(_no_point_x(ec)) + sigs[8][32:]
    pool_status = nat.excess_verify_each(files, ss, en, public, msgs, sigs)
    assert [pool_status[t] for t in (2, 6, 8)] == [NOT_CANONICAL, BAD_R, BAD_R]
    assert nat.excess_verify_keys_each(keys, msgs, sigs) == pool_status
    assert nat.excess_verify_keys_batch(keys, msgs, sigs, SEED, want_status=True)[:2] == (False, pool_status)


# ----------------------------------------------------------------------------- 4. the weighted combination over stated keys
@pytest.mark.parametrize("name", ["rec_test", "bin_test"])
def test_keys_batch(gpu, oracle_lib, handles, name):
    st = _case(oracle_lib, name)[0]
    nat, be, ec, B = handles(name), OracleBackend(oracle_lib), oracle_lib, _blind_base(_case(oracle_lib, name)[0], name)
    n = 101
    es, msgs = _scalars(n, 41), _msgs(n, b"batch")
    sigs, keys = nat.excess_sign(es, msgs, AUX), nat.excess_keys(es)
    assert nat.excess_verify_keys_batch(keys, msgs, sigs, SEED, want_status=True, want_point=True) == (True, [OK] * n, None)
    assert nat.excess_verify_keys_batch(keys, msgs, sigs) is True                       # a fresh seed
    bad = list(sigs)
    bad[70] = _with_s(sigs[70], (_s_of(sigs[70]) + 1) % N)
    each = nat.excess_verify_keys_each(keys, msgs, bad)
    assert each == [MISMATCH if t == 70 else OK for t in range(n)]
    want = _combined_keys(ec, B, SEED, 0, keys, msgs, bad, 0, n)
    assert nat.excess_verify_keys_batch(keys, msgs, bad, SEED, want_status=True, want_point=True) == (False, each, want) and want is not None
    other = nat.excess_verify_keys_batch(keys, msgs, bad, hashlib.sha256(b"another").digest(), want_point=True)
    assert other[0] is False and other[2] not in (None, want)
    # a key that does not lift puts in no term: the point is the identity and the batch still rejects
    bad_keys = list(keys)
    bad_keys[5] = keys[5][:32] + b"\x02"
    each = [BAD_KEY if t == 5 else OK for t in range(n)]
    assert nat.excess_verify_keys_batch(bad_keys, msgs, sigs, SEED, want_status=True, want_point=True) == (False, each, None)
    assert nat.excess_verify_keys_batch(bad_keys, msgs, sigs, SEED) is False
    # host = _device; two shards of one job add up to the one-call point; another offset is another point
    with _Dev(gpu, k=_bytes(keys), m=_bytes(msgs), g=_bytes(bad)) as d:
        assert nat.excess_verify_keys_batch_device(n, d["k"], d["m"], d["g"], seed=SEED, want_status=True, want_point=True)[::2] == (False, want)
        acc7, _, p7 = nat.excess_verify_keys_batch_device(n, d["k"], d["m"], d["g"], seed=SEED, index_offset=2**32 + 7, want_point=True)
        assert not acc7 and p7 == _combined_keys(ec, B, SEED, 2**32 + 7, keys, msgs, bad, 0, n) and p7 != want
    parts = []
    for lo, hi in ((0, 37), (37, n)):
        with _Dev(gpu, k=_bytes(keys[lo:hi]), m=_bytes(msgs[lo:hi]), g=_bytes(bad[lo:hi])) as d:
            ak, _, pk = nat.excess_verify_keys_batch_device(hi - lo, d["k"], d["m"], d["g"], seed=SEED, index_offset=lo, want_point=True)
        assert ak == (lo == 0) and pk == (None if lo == 0 else want)
        parts.append(pk)
    assert gpu.sum_points(capi.points_to_array(parts)) == want
    acc0 = C.c_int(-1)
    assert gpu.lib.bppp_rp_excess_verify_keys_batch_device(nat.h, 0, None, None, None, 9, None, C.byref(acc0), None, None) == 0 and acc0.value == 1
    status = np.full(2, 0xA5A5A5A5, dtype=np.uint32)
    assert gpu.lib.bppp_rp_excess_verify_keys_each(nat.h, 2, None, None, None, C.c_void_p(status.ctypes.data)) == -1 and b"null input" in gpu.lib.bppp_last_error(gpu.h)
    assert (status == 0xA5A5A5A5).all()


# ----------------------------------------------------------------------------- 5. sums against stated keys, sum by sum
def _sums_job(oracle_lib, name, seed, broken_j=None, zero_claims=False):
    """one sum per SHAPES entry, balanced: the claim is tally_claims_host's with the blinding sum split into the offset and the keys' scalars"""
    st, inputs, triples, flat, files = _pool(oracle_lib, name)
    ec, B, rng = oracle_lib, _blind_base(st, name), random.Random(seed)
    pick = [j for j in range(len(flat)) if j != broken_j]
    sums = [[(rng.choice(pick), i % 2 == 1 if ne > 1 else rng.random() < 0.5) for i in range(ne)] for ne, _ in SHAPES]       # both signs in every longer sum
    ss, en = _csr(sums)
    ks = [[rng.randrange(1, N) for _ in range(nk)] for _, nk in SHAPES]
    key_start = [0]
    for k in ks:
        key_start.append(key_start[-1] + len(k))
    keys = [RP.excess_key33(ec.mul(k, B)) for group in ks for k in group]
    claims = [(a, ty, (e - sum(group)) % N) for (a, ty, e), group in zip(RP.tally_claims_host(triples, ss, en), ks)]
    return st, flat, files, ss, en, claims, key_start, keys


def _host_sums(be, st, name, flat, ss, en, claims, key_start, keys, broken=()):
    S = RP.tally_sums(be, flat, ss, en)
    out = []
    for t in range(len(ss) - 1):
        claim = (0, 0, 0) if claims is None else claims[t]
        claim = claim if name != "bin_test" else (claim[0], claim[-1])
        out.append(RP.excess_sums_host(be, st, S[t], claim, keys[key_start[t]:key_start[t + 1]], malformed=any((e & (SUB - 1)) in broken for e in en[ss[t]:ss[t + 1]])))
    return [v for v, _ in out], [p for _, p in out]


def _native_claims(name, claims):
    return claims if claims is None or name != "bin_test" else [(a, o) for a, _, o in claims]


def _sums_dev(nat, files, ss, en, claims, key_start, keys, alloc=None):
    ssa, ena, nsums, nnz = nat._tally_csr(ss, en)
    amt, typ, off = nat._tally_claim_arrays(claims, nsums)
    dev = _Dev(alloc or nat.gpu, cf=_bytes(files), ss=ssa, en=ena, amt=amt, typ=typ if nat.st.__class__.__name__ == "SetupTRRP" else None, off=off,
               ks=np.array(key_start, dtype=np.uint32), ky=_bytes(keys))
    return dev, lambda d: (len(files), d["cf"], nsums, d["ss"], d["en"], nnz, d["amt"], d["typ"], d["off"], len(keys), d["ks"], d["ky"])


def _sums_each_both(nat, files, ss, en, claims, key_start, keys):
    host = nat.excess_sums_each(files, ss, en, claims, key_start, keys, want_points=True)
    dev, args = _sums_dev(nat, files, ss, en, claims, key_start, keys)
    with dev as d:
        assert nat.excess_sums_each_device(*args(d), want_points=True) == host
    return host


@pytest.mark.parametrize("name", NAMES)
def test_sums_each(gpu, oracle_lib, handles, hooks, name):
    nat, be = handles(name), OracleBackend(oracle_lib)
    st, flat, files, ss, en, claims, key_start, keys = _sums_job(oracle_lib, name, 51)
    nsums = len(SHAPES)
    tampered = list(claims)
    tampered[4] = ((claims[4][0] + 1) % N,) + claims[4][1:]                             # an amount
    tampered[6] = claims[6][:2] + ((claims[6][2] + 1) % N,)                             # an offset
    if name not in ("bin_test",):
        tampered[5] = (claims[5][0], (claims[5][1] + 1) % N, claims[5][2])             # a type: typed handles only
    swapped = list(keys)
    swapped[key_start[7]], swapped[key_start[3]] = keys[key_start[3]], keys[key_start[7]]       # a key of sum 7 and the key of sum 3 change places
    jobs = [(claims, keys), (tampered, keys), (claims, swapped), (None, keys)]
    wants = [_host_sums(be, st, name, flat, ss, en, c, key_start, k) for c, k in jobs]
    assert wants[0][0] == [OK] * nsums
    assert wants[1][0] == [MISMATCH if t in ((4, 6) if name == "bin_test" else (4, 5, 6)) else OK for t in range(nsums)]
    assert wants[2][0] == [MISMATCH if t in (3, 7) else OK for t in range(nsums)]
    assert wants[3][0][0] == OK and wants[3][0][7] == MISMATCH                          # zero claims: the empty sum balances, the others hardly
    for small in (False, True):
        if small:
            hooks(nat, short_max=4, piece=8, chunk=64)                                  # the lane route, the piece route with a key group across a piece edge, several passes
        for (c, k), want in zip(jobs, wants):
            assert _sums_each_both(nat, files, ss, en, _native_claims(name, c), key_start, k) == tuple(want), small
        assert nat.excess_sums_each(files, ss, en, _native_claims(name, claims), key_start, keys) == wants[0][0]
    hooks(nat)
    # no keys at all: the tally, with the offset as the claimed blinding
    none = [0] * (nsums + 1)
    want = _host_sums(be, st, name, flat, ss, en, claims, none, [])
    assert want[0][0] == OK and want[0][7] == MISMATCH
    assert _sums_each_both(nat, files, ss, en, _native_claims(name, claims), none, []) == tuple(want)
    assert nat.tally_each(files, ss, en, _native_claims(name, claims), want_points=True) == tuple(want)


@pytest.mark.parametrize("name", ["rec_test", "bin_test"])
def test_sums_verdict_precedence(gpu, oracle_lib, handles, name):
    nat, be, typed = handles(name), OracleBackend(oracle_lib), name != "bin_test"
    nr = len(_case(oracle_lib, name)[0].rds)
    broken_j = 2 * nr + min(1, nr - 1)
    st, flat, files, ss, en, claims, key_start, keys = _sums_job(oracle_lib, name, 61, broken_j=broken_j)
    bx = _no_point_x(oracle_lib)
    broken = list(files)
    broken[2] = _set_x(files[2], nr, min(1, nr - 1), bx)
    # sum 4: a commitment without a point, a key without a point and an offset >= n; sum 5: the key and the offset; sum 6: the offset; sum 7: a key's x
    en[ss[4]] = RP.tally_entry(broken_j, True)
    keys[key_start[4]] = keys[key_start[4]][:32] + b"\x02"
    keys[key_start[5] + 16] = keys[key_start[5] + 16][:32] + b"\x05"                    # the last key of its group
    keys[key_start[7] + 13] = RP._put(bx) + b"\x01"
    for t in (4, 5, 6):
        claims[t] = claims[t][:2] + (N,)
    want = _host_sums(be, st, name, flat, ss, en, claims, key_start, keys, broken=(broken_j,))
    assert want[0] == [OK, OK, OK, OK, MALFORMED, BAD_KEY, NOT_CANONICAL, BAD_KEY] and want[1][4] is None and want[1][5] is None and want[1][6] is not None
    assert _sums_each_both(nat, broken, ss, en, _native_claims(name, claims), key_start, keys) == tuple(want)
    acc, status, _ = nat.excess_sums_batch(broken, ss, en, _native_claims(name, claims), key_start, keys, SEED, want_status=True)
    assert not acc and status == want[0]
    # a key without a point alone: nothing malformed, nothing non-canonical, and the batch still rejects
    st, flat, files, ss, en, claims, key_start, keys = _sums_job(oracle_lib, name, 61)
    keys[key_start[7] + 39] = keys[key_start[7] + 39][:32] + b"\x02"
    want = [BAD_KEY if t == 7 else OK for t in range(len(SHAPES))]
    assert nat.excess_sums_batch(files, ss, en, _native_claims(name, claims), key_start, keys, SEED, want_status=True)[:2] == (False, want)
    if typed:
        claims[1] = (claims[1][0], N, claims[1][2])
        want[1] = NOT_CANONICAL
        assert nat.excess_sums_each(files, ss, en, claims, key_start, keys) == want


# ----------------------------------------------------------------------------- 6. the weighted combination over sums and keys
@pytest.mark.parametrize("name", ["rec_test", "bin_test"])
def test_sums_batch(gpu, oracle_lib, handles, hooks, name):
    nat, be, ec, typed = handles(name), OracleBackend(oracle_lib), oracle_lib, name != "bin_test"
    st, flat, files, ss, en, claims, key_start, keys = _sums_job(oracle_lib, name, 71)
    g, H0, B = RP._excess_bases(st)
    nsums = len(SHAPES)
    nc = _native_claims(name, claims)
    assert nat.excess_sums_batch(files, ss, en, nc, key_start, keys, SEED, want_status=True, want_point=True) == (True, [OK] * nsums, None)
    assert nat.excess_sums_batch(files, ss, en, nc, key_start, keys) is True
    bad = list(claims)
    bad[3] = ((claims[3][0] + 1) % N,) + claims[3][1:]
    bad[7] = claims[7][:2] + ((claims[7][2] + 5) % N,)
    nb = _native_claims(name, bad)
    S = RP.tally_sums(be, flat, ss, en)

    def combined(offset, lo, hi):
        """sum over t in [lo, hi) of rho_t (S_t - a_t g - ty_t H0 - o_t B - the keys of group t), by the oracle"""
        terms = []
        for t in range(lo, hi):
            a, ty, o = bad[t]
            rho = RP.tally_weight(SEED, offset + t, a, ty if typed else 0, o)
            terms += [(rho, S[t]), ((-rho * a) % N, g), ((-rho * o) % N, B)] + ([((-rho * ty) % N, H0)] if typed else [])
            terms += [((-rho) % N, _lift(ec, k)) for k in keys[key_start[t]:key_start[t + 1]]]
        return ec.inner_product([(s, p) for s, p in terms if p is not None and s])
    want = combined(0, 0, nsums)
    each = nat.excess_sums_each(files, ss, en, nb, key_start, keys)
    assert each == [MISMATCH if t in (3, 7) else OK for t in range(nsums)]
    for small in (False, True):
        if small:
            hooks(nat, short_max=4, piece=8, chunk=64)                                  # several MSMs, the long sum in pieces of one pass
        assert nat.excess_sums_batch(files, ss, en, nb, key_start, keys, SEED, want_status=True, want_point=True) == (False, each, want) and want is not None
    hooks(nat)
    dev, args = _sums_dev(nat, files, ss, en, nb, key_start, keys)
    with dev as d:
        assert nat.excess_sums_batch_device(*args(d), seed=SEED, want_status=True, want_point=True) == (False, each, want)
        acc7, _, p7 = nat.excess_sums_batch_device(*args(d), seed=SEED, index_offset=2**32 + 7, want_point=True)
        assert not acc7 and p7 == combined(2**32 + 7, 0, nsums) and p7 != want
    parts = []
    for lo, hi in ((0, 4), (4, 7), (7, nsums)):
        ssk, ksk = [v - ss[lo] for v in ss[lo:hi + 1]], [v - key_start[lo] for v in key_start[lo:hi + 1]]
        dk, ak = _sums_dev(nat, files, ssk, en[ss[lo]:ss[hi]], nb[lo:hi], ksk, keys[key_start[lo]:key_start[hi]])
        with dk as d:
            acc, _, pk = nat.excess_sums_batch_device(*ak(d), seed=SEED, index_offset=lo, want_point=True)
        assert pk == combined(0, lo, hi) and acc == (lo == 4)
        parts.append(pk)
    assert parts[1] is None and gpu.sum_points(capi.points_to_array(parts)) == want
    acc0 = C.c_int(-1)
    assert gpu.lib.bppp_rp_excess_sums_batch_device(nat.h, 0, None, 0, None, None, 0, None, None, None, 0, None, None, 9, None, C.byref(acc0), None, None) == 0 and acc0.value == 1
    assert gpu.lib.bppp_rp_excess_sums_each(nat.h, 0, None, 0, None, None, 0, None, None, None, 0, None, None, None, None) == 0


# ----------------------------------------------------------------------------- 7. argument errors: an error code, and no output is written
def test_sums_errors(gpu, oracle_lib, handles):
    nat, lib = handles("rec_test"), gpu.lib
    st, flat, files, ss, en, claims, key_start, keys = _sums_job(oracle_lib, "rec_test", 81)
    nsums, nkeys, nnz = len(SHAPES), len(keys), len(en)
    down = list(key_start)
    down[5] = down[4] - 1
    short = key_start[:-1] + [nkeys - 1]
    for bad_ks, msg in ((down, r"rp_excess_sums_\w+: key_start\[5\] = %d " % down[5]), (short, r"rp_excess_sums_\w+: key_start\[%d\] = %d .*nkeys = %d" % (nsums, nkeys - 1, nkeys))):
        with pytest.raises(capi.BpppError, match=msg):
            nat.excess_sums_each(files, ss, en, claims, bad_ks, keys)
        with pytest.raises(capi.BpppError, match=msg):
            nat.excess_sums_batch(files, ss, en, claims, bad_ks, keys, SEED)
    with pytest.raises(capi.BpppError, match=r"rp_excess_sums_each: sum_start\[2\] = "):
        nat.excess_sums_each(files, [0, 1, 0] + ss[3:], en, claims, key_start, keys)
    dev, args = _sums_dev(nat, files, ss, en, claims, key_start, keys)
    with dev as d:
        a = args(d)
        p = [C.c_void_p(v) if i in (1, 3, 4, 6, 7, 8, 10, 11) else v for i, v in enumerate(a)]
        status, xy, acc = np.full(nsums, 0xA5A5A5A5, dtype=np.uint32), np.full((nsums, 8), 0xA5, dtype=np.uint64), C.c_int(-1)
        vp = lambda x: C.c_void_p(x.ctypes.data)
        sd = vp(np.frombuffer(SEED, dtype=np.uint8))
        with _Dev(gpu, down=np.array(down, dtype=np.uint32), short=np.array(short, dtype=np.uint32)) as bad:
            for k in ("down", "short"):
                q = list(p)
                q[10] = C.c_void_p(bad[k])
                assert lib.bppp_rp_excess_sums_each_device(nat.h, *q, vp(status), vp(xy)) == -1 and b"key_start[" in lib.bppp_last_error(gpu.h)
                assert lib.bppp_rp_excess_sums_batch_device(nat.h, *q, 0, sd, C.byref(acc), vp(status), vp(xy)) == -1 and b"key_start[" in lib.bppp_last_error(gpu.h)
        q = list(p)
        q[9] = 2**31 - len(flat)                                                        # rows * nranges + nkeys = 2^31: refused before anything is read
        assert lib.bppp_rp_excess_sums_each_device(nat.h, *q, vp(status), vp(xy)) == -1 and b"rows * nranges + nkeys must be below 2^31" in lib.bppp_last_error(gpu.h)
        assert lib.bppp_rp_excess_sums_batch_device(nat.h, *q, 0, sd, C.byref(acc), vp(status), vp(xy)) == -1
        q[9] = 2**31 - nnz                                                              # nnz + nkeys = 2^31 (and the first limit broken too)
        assert lib.bppp_rp_excess_sums_each_device(nat.h, *q, vp(status), vp(xy)) == -1
        for drop in ((6,), (7,), (8,), (6, 8), (7, 8)):                                 # only some of the three claim arrays
            q = list(p)
            for k in drop:
                q[k] = None
            assert lib.bppp_rp_excess_sums_each_device(nat.h, *q, vp(status), vp(xy)) == -1 and b"claim_offsets must be given together" in lib.bppp_last_error(gpu.h)
        for k in (1, 3, 4, 10, 11):                                                     # NULL buffers
            q = list(p)
            q[k] = None
            assert lib.bppp_rp_excess_sums_each_device(nat.h, *q, vp(status), vp(xy)) == -1 and b"null input" in lib.bppp_last_error(gpu.h)
        assert lib.bppp_rp_excess_sums_each_device(nat.h, *p, None, None) == -1
        assert lib.bppp_rp_excess_sums_batch_device(nat.h, *p, 0, None, C.byref(acc), vp(status), vp(xy)) == -1
        assert (status == 0xA5A5A5A5).all() and (xy == 0xA5).all() and acc.value == 0
        assert lib.bppp_rp_excess_sums_each_device(nat.h, *p, vp(status), None) == 0 and list(status) == [OK] * nsums
    # the host variant refuses the sizes before it uploads: the key array here is one row, not 2^31
    cf, two, one = _bytes(files), np.zeros(2, dtype=np.uint32), np.zeros(KEY, dtype=np.uint8)
    assert lib.bppp_rp_excess_sums_each(nat.h, len(files), vp(cf), 1, vp(two), None, 0, None, None, None, 2**31, vp(two), vp(one), vp(status), None) == -1
    assert b"nkeys must be below 2^31" in lib.bppp_last_error(gpu.h)


# ----------------------------------------------------------------------------- 8. cut-through, through the native calls
@pytest.mark.parametrize("name", ["32bit", "bin_test"])
def test_cut_through(gpu, oracle_lib, handles, name):
    """Transaction 1 spends A into B and C, transaction 2 spends B into D; each builder splits its blinding sum into a revealed offset and a signing
    key.  The block keeps - A + C + D, the summed claim and the summed offset: B is gone from its pool."""
    st, inputs, triples, flat, files = _pool(oracle_lib, name)
    nat = handles(name)
    nr = len(st.rds)
    A, B, Cc, D = 0, nr, 2 * nr, 3 * nr                                                 # the first commitment of rows 0 .. 3
    tx_ss, tx_en = _csr([[(A, True), (B, False), (Cc, False)], [(B, True), (D, False)]])
    (a1, ty1, e1), (a2, ty2, e2) = RP.tally_claims_host(triples, tx_ss, tx_en)           # a = minus the fee of each
    o1, o2 = _scalars(2, 91)
    k = [(e1 - o1) % N, (e2 - o2) % N]
    keys, msgs = nat.excess_keys(k), _msgs(2, b"cut through")
    sigs = nat.excess_sign(k, msgs, AUX)
    pool = [files[0], files[2], files[3]]                                               # no row of B
    ss, en = _csr([[(0, True), (nr, False), (2 * nr, False)]])
    claim = ((a1 + a2) % N, (ty1 + ty2) % N, (o1 + o2) % N)
    nc = lambda c: [c if name != "bin_test" else (c[0], c[2])]
    assert nat.excess_verify_keys_batch(keys, msgs, sigs, SEED, want_status=True) == (True, [OK, OK], None)
    assert nat.excess_sums_each(pool, ss, en, nc(claim), [0, 2], keys) == [OK]
    assert nat.excess_sums_batch(pool, ss, en, nc(claim), [0, 2], keys, SEED, want_status=True) == (True, [OK], None)
    # one tamper at a time, each caught by the call that should catch it
    assert nat.excess_sums_each(pool, ss, en, nc(claim), [0, 1], keys[:1]) == [MISMATCH]                    # a key left out
    assert nat.excess_sums_batch(pool, ss, en, nc(claim), [0, 1], keys[:1], SEED) is False
    off = ((claim[0] + 1) % N,) + claim[1:]
    assert nat.excess_sums_each(pool, ss, en, nc(off), [0, 2], keys) == [MISMATCH]                          # a fee off by one
    assert nat.excess_sums_batch(pool, ss, en, nc(off), [0, 2], keys, SEED, want_status=True)[:2] == (False, [MISMATCH])
    assert nat.excess_verify_keys_each(keys[::-1], msgs, sigs) == [MISMATCH, MISMATCH]                      # signatures under the other transaction's key
    assert nat.excess_verify_keys_batch(keys[::-1], msgs, sigs, SEED) is False
    assert nat.excess_sums_each(pool, ss, en, nc(claim), [0, 2], keys[::-1]) == [OK]                        # the sum does not care which key is whose
    other = nat.excess_keys([(k[0] + 1) % N])
    assert nat.excess_sums_each(pool, ss, en, nc(claim), [0, 2], [other[0], keys[1]]) == [MISMATCH]         # a key that was not the builder's
    assert nat.excess_sums_each(files[:4], ss, en, nc(claim), [0, 2], keys) == [MISMATCH]                   # the pool with B still in it names other rows
