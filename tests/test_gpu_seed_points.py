"""bppp_points_from_seed{,_device} and the seeded handle constructors: getPoints (app/Main.hs:68-72) on the GPU.  The expected stream is
restated inline — SHA-256 (seed <> decimal n), the digest read as four big-endian 64-bit words with the least significant first, mod p,
kept when x^3 + 7 is a square, y = the even root by pow(rhs, (p + 1) // 4, p) — and asserted equal to rangeproof.basis_points as well.
Sizes: 130 points pass the 9 -> 10 and 99 -> 100 digit edges, 600 pass 999 -> 1000; forced chunks of 64 and 256 candidates give many
passes and takes across wavefront and workgroup edges (a workgroup is 256 candidates); 10^19 - 4 reaches twenty digits."""
import ctypes as C
import functools
import hashlib
import json
import os
import random

import numpy as np
import pytest

from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import BpppError, array_to_point, load_test_library, scalars_to_array
from test_rangeproof import EXAMPLES

pytestmark = pytest.mark.gpu

P = 2**256 - 2**32 - 977
TP = b"test points"
SEEDS = [TP, b"", b"s" * 55, b"s" * 56, b"s" * 64, b"s" * 65, bytes(range(120))]
VSEED = hashlib.sha256(b"seeded handles").digest()


def _decode(digest):
    return sum(int.from_bytes(digest[8 * i:8 * i + 8], "big") << (64 * i) for i in range(4)) % P


def _lift(x):
    rhs = (x * x * x + 7) % P
    y = pow(rhs, (P + 1) // 4, P)
    if y * y % P != rhs:
        return None
    return (x, P - y if y & 1 else y)


@functools.lru_cache(maxsize=None)
def _stream(seed, count, first=0):
    """([(candidate index, point)] of the first `count` accepted candidates from `first`)"""
    out, n = [], first
    while len(out) < count:
        pt = _lift(_decode(hashlib.sha256(seed + str(n).encode()).digest()))
        if pt is not None:
            out.append((n, pt))
        n += 1
    return tuple(out)


def _points(arr):
    return [array_to_point(r) for r in arr]


def test_the_restatement_is_basis_points():
    for seed in SEEDS:
        assert [pt for _, pt in _stream(seed, 130)] == RP.basis_points(seed, 130)
    assert [pt for _, pt in _stream(TP, 600)] == RP.basis_points(TP, 600)


# ----------------------------------------------------------------------------- 1. stream equality
@pytest.mark.parametrize("seed", SEEDS, ids=lambda s: "len%d" % len(s))
def test_stream_equality(gpu, seed):
    want = _stream(seed, 130)
    assert want[-1][0] >= 100                                   # three-digit candidates are reached
    got, nxt = gpu.points_from_seed(seed, 130)
    assert _points(got) == [pt for _, pt in want]
    assert nxt == want[-1][0] + 1


def test_stream_equality_600(gpu):
    want = _stream(TP, 600)
    got, nxt = gpu.points_from_seed(TP, 600)
    assert _points(got) == [pt for _, pt in want]
    assert nxt == want[-1][0] + 1 == 1160


def test_pins(gpu):
    for count, nxt in [(1, 1), (64, 115), (65, 116), (600, 1160)]:
        assert _stream(TP, count)[-1][0] + 1 == nxt
        assert gpu.points_from_seed(TP, count)[1] == nxt
    assert _stream(b"", 1)[0][0] == 2 and gpu.points_from_seed(b"", 1)[1] == 3
    assert _stream(b"s" * 64, 1)[0][0] == 4 and gpu.points_from_seed(b"s" * 64, 1)[1] == 5


# ----------------------------------------------------------------------------- 2. resumption and offsets
def test_resumption(gpu):
    a, na = gpu.points_from_seed(TP, 65)
    b, nb = gpu.points_from_seed(TP, 70, first_candidate=na)
    whole, nw = gpu.points_from_seed(TP, 135)
    assert np.array_equal(np.concatenate([a, b]), whole) and nb == nw
    assert _points(whole) == [pt for _, pt in _stream(TP, 135)]


def test_first_candidate_that_does_not_lift(gpu):
    assert [n for n, _ in _stream(TP, 2)] == [0, 2]             # candidate 1 does not lift
    got, nxt = gpu.points_from_seed(TP, 3, first_candidate=1)
    want = _stream(TP, 3, 1)
    assert want[0][0] == 2 and _points(got) == [pt for _, pt in want] and nxt == want[-1][0] + 1


def test_count_zero_writes_nothing(gpu):
    out = np.full((2, 8), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    nxt = C.c_uint64(0)
    gpu._check(gpu.lib.bppp_points_from_seed(gpu.h, TP, len(TP), 77, 0, C.c_void_p(out.ctypes.data), C.byref(nxt)), "bppp_points_from_seed")
    assert nxt.value == 77 and (out == 0x5A5A5A5A5A5A5A5A).all()
    d = gpu.to_device(out)
    try:
        nxt = C.c_uint64(0)
        gpu._check(gpu.lib.bppp_points_from_seed_device(gpu.h, None, 0, 2**64 - 1, 0, C.c_void_p(d), C.byref(nxt)), "bppp_points_from_seed_device")
        assert nxt.value == 2**64 - 1 and np.array_equal(gpu.download(d, (2, 8)), out)
        gpu._check(gpu.lib.bppp_points_from_seed_device(gpu.h, TP, len(TP), 5, 0, None, None), "bppp_points_from_seed_device")
    finally:
        gpu.free(d)


# ----------------------------------------------------------------------------- 3. twenty-digit indices
def test_twenty_digit_candidates(gpu):
    first = 10**19 - 4
    want = _stream(TP, 8, first)
    assert want[-1][0] >= 10**19
    got, nxt = gpu.points_from_seed(TP, 8, first_candidate=first)
    assert _points(got) == [pt for _, pt in want] and nxt == want[-1][0] + 1


def test_search_past_the_last_candidate(gpu):
    with pytest.raises(BpppError) as e:
        gpu.points_from_seed(TP, 8, first_candidate=2**64 - 4)
    assert "(-1)" in str(e.value)
    with pytest.raises(BpppError) as e:
        gpu.points_from_seed(TP, 600, first_candidate=2**64 - 700, device=True)
    assert "(-1)" in str(e.value)
    assert gpu.points_from_seed(TP, 1)[1] == 1                   # the context still works


def test_argument_errors(gpu):
    out = np.zeros((4, 8), dtype=np.uint64)
    lib = gpu.lib
    assert lib.bppp_points_from_seed(gpu.h, b"s" * 4097, 4097, 0, 4, C.c_void_p(out.ctypes.data), None) == -1
    assert lib.bppp_points_from_seed(gpu.h, None, 3, 0, 4, C.c_void_p(out.ctypes.data), None) == -1
    assert lib.bppp_points_from_seed(gpu.h, TP, len(TP), 0, 4, None, None) == -1
    assert lib.bppp_points_from_seed_device(gpu.h, TP, len(TP), 0, 4, None, None) == -1
    assert lib.bppp_points_from_seed(None, TP, len(TP), 0, 4, C.c_void_p(out.ctypes.data), None) == -1
    assert not out.any()
    import bulletproofspp_amd as b
    ctx = b.Bppp(0)
    h = ctx.h
    basis = ctx.basis(np.ascontiguousarray(gpu.points_from_seed(TP, 2)[0]))      # keeps the closed context's memory alive
    lib.bppp_ctx_destroy(h)
    ctx.h = None
    assert lib.bppp_points_from_seed(h, TP, len(TP), 0, 4, C.c_void_p(out.ctypes.data), None) == -1
    basis.close()


# ----------------------------------------------------------------------------- 4. pass and workgroup boundaries
@pytest.mark.parametrize("chunk", [64, 256])
def test_forced_chunks(gpu, chunk):
    tl = load_test_library()
    out = np.zeros((300, 8), dtype=np.uint64)
    nxt = C.c_uint64(0)
    gpu._check(tl.bppp_test_points_from_seed_chunked(gpu.h, TP, len(TP), 0, 300, chunk, C.c_void_p(out.ctypes.data), C.byref(nxt)), "chunked")
    one, n1 = gpu.points_from_seed(TP, 300)
    want = _stream(TP, 300)
    assert want[-1][0] + 1 > 2 * chunk                           # several passes
    assert np.array_equal(out, one) and nxt.value == n1 == want[-1][0] + 1
    assert _points(out) == [pt for _, pt in want]


# ----------------------------------------------------------------------------- 5. r >= p
def test_digests_at_and_above_the_modulus(gpu):
    tl = load_test_library()
    rs = [P, P + 1, P + 2, 2**256 - 1, P - 1, 5]
    digests = b"".join(b"".join(((r >> (64 * i)) & (2**64 - 1)).to_bytes(8, "big") for i in range(4)) for r in rs)
    assert [_decode(digests[32 * k:32 * k + 32]) for k in range(4)] == [0, 1, 2, 2**256 - 1 - P]
    n = len(rs)
    x, ok, pts = np.zeros((n, 4), dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros((n, 8), dtype=np.uint64)
    gpu._check(tl.bppp_test_seed_lift_digests(gpu.h, digests, n, C.c_void_p(x.ctypes.data), C.c_void_p(ok.ctypes.data), C.c_void_p(pts.ctypes.data)), "lift_digests")
    for k, r in enumerate(rs):
        want = _lift(r % P)
        assert int(sum(int(v) << (64 * j) for j, v in enumerate(x[k]))) == r % P, k
        assert bool(ok[k]) == (want is not None), k
        assert array_to_point(pts[k]) == want, k
    assert any(ok[:4]) and not all(ok[:4])                       # both outcomes occur among the four


# ----------------------------------------------------------------------------- 6. determinism and curve
def test_determinism_and_curve(gpu, oracle_lib):
    a, na = gpu.points_from_seed(TP, 600)
    b, nb = gpu.points_from_seed(TP, 600)
    assert a.tobytes() == b.tobytes() and na == nb
    pts = _points(a[::9][:64])
    assert len(pts) == 64
    for pt in pts:
        assert pt is not None and oracle_lib.on_curve(pt) and pt[1] % 2 == 0


# ----------------------------------------------------------------------------- 7. device output feeds the rest
def test_device_points_feed_a_basis_and_an_msm(gpu, oracle_lib):
    import pyoracle as O
    n = 1000
    rnd = random.Random(7)
    sc = [rnd.randrange(O.N) for _ in range(n)]
    d_pts, nxt = gpu.points_from_seed(TP, n, device=True)
    d_sc = gpu.to_device(scalars_to_array(sc))
    try:
        want_pts = [pt for _, pt in _stream(TP, n)]
        assert nxt == _stream(TP, n)[-1][0] + 1
        basis = gpu.basis(d_pts, device=True, n=n)
        got = basis.msm(d_sc, n)[0]
        basis.close()
        assert got == oracle_lib.inner_product(list(zip(sc, want_pts)))
    finally:
        gpu.free(d_pts); gpu.free(d_sc)


# ----------------------------------------------------------------------------- 8. seeded handles
def _schema(name):
    return json.load(open(os.path.join(EXAMPLES, name, "schema.json")))


def _handle(gpu, name, seeded, basis_seed=None):
    schema = _schema(name)
    if basis_seed is not None:
        schema["basisSeed"] = basis_seed
    seed = str(schema["basisSeed"]).encode() if seeded else None
    if schema.get("binary", False):
        return BRP.NativeBinaryRangeProofs(gpu, BRP.setup_from_schema(RP.GpuBackend(gpu), schema), basis_seed=seed)
    return RP.NativeRangeProofs(gpu, RP.setup_from_schema(RP.GpuBackend(gpu), schema), basis_seed=seed)


def _inputs(name, count):
    wit = json.load(open(os.path.join(EXAMPLES, name, "witness.json")))
    binary = bool(_schema(name).get("binary", False))
    rows = [RP.inputs_from_witness(wit, b"seeded %s %d" % (name.encode(), j)) for j in range(count)]
    return [[(v, bl) for v, _, bl in r] for r in rows] if binary else rows


def _prefixes(count):
    return [b"seeded random seed %d" % j for j in range(count)]


@pytest.mark.parametrize("name", ["32bit", "bin_test"])
def test_seeded_handle_is_the_unseeded_one(gpu, name):
    assert _schema(name)["basisSeed"] == "test points"
    seeded, plain = _handle(gpu, name, True), _handle(gpu, name, False)
    try:
        assert seeded.shape == plain.shape
        inputs, prefixes = _inputs(name, 2), _prefixes(2)
        fa, fb = seeded.prove_batch(inputs, prefixes), plain.prove_batch(inputs, prefixes)
        assert fa == fb
        assert plain.verify_batch([c for c, _ in fa], [p for _, p in fa], VSEED)
        assert seeded.verify_batch([c for c, _ in fb], [p for _, p in fb], VSEED)
        bad = bytearray(fb[1][1]); bad[5] ^= 1
        assert seeded.verify_batch([c for c, _ in fb], [fb[0][1], bytes(bad)], VSEED, want_status=True)[:2] == (False, [0, 1])
    finally:
        seeded.close(); plain.close()


def test_seeded_handles_form_one_family(gpu):
    short, long, other = _handle(gpu, "32bit", True), _handle(gpu, "32by64", True), _handle(gpu, "32by64", True, basis_seed="other points")
    tl = load_test_library()
    try:
        for h in (short, long, other):
            h.set_option("comb_min", 1); h.set_option("comb_bits", 6)
        assert long.shape["norm_len"] + long.shape["lin_len"] > short.shape["norm_len"] + short.shape["lin_len"]
        short.share_comb(long)
        info = short.comb_info()
        assert info == long.comb_info() and info["users"] == 2 and info["points"] == 1 + long.shape["lin_len"] + long.shape["norm_len"]
        with pytest.raises(BpppError) as e:
            short.share_comb(other)
        assert "(-1)" in str(e.value) and "extend" in str(e.value)
        fs = short.prove_batch(_inputs("32bit", 2), _prefixes(2))
        fl = long.prove_batch(_inputs("32by64", 2), _prefixes(2))
        groups = [(short, [c for c, _ in fs], [p for _, p in fs]), (long, [c for c, _ in fl], [p for _, p in fl])]
        assert RP.verify_mixed(gpu, groups, VSEED, want_status=True) == (True, [0] * 4)
        terms = C.c_uint64(0)
        assert tl.bppp_test_last_mixed_msm_terms(gpu.h, C.byref(terms)) == 0
        per = sum(2 * (4 + h.shape["nranges"] + 2 * h.shape["rounds"]) for h in (short, long))
        assert terms.value == 1 + long.shape["lin_len"] + long.shape["norm_len"] + per        # the shorter basis was merged into the longer
    finally:
        short.close(); long.close(); other.close()


def test_seeded_constructor_keeps_the_counterparts_errors(gpu):
    from bulletproofspp_amd.capi import RpRange, int_to_limbs
    rng = (RpRange * 1)()
    rng[0].base = 16
    rng[0].max[:] = [int(v) for v in int_to_limbs(2**64)]
    h = C.c_void_p()
    lib = gpu.lib
    args = (C.cast(rng, C.c_void_p), 1, None, 0)
    assert lib.bppp_rp_create_seeded(gpu.h, 2, 0, *args, TP, len(TP), None, C.byref(h)) == -1
    assert b"flavour" in lib.bppp_last_error(gpu.h)
    assert lib.bppp_rp_create_seeded(gpu.h, 0, 0, *args, b"s" * 4097, 4097, None, C.byref(h)) == -1
    assert b"seed" in lib.bppp_last_error(gpu.h) and not h.value
    rng[0].base = 1
    assert lib.bppp_rp_create_seeded(gpu.h, 0, 0, *args, TP, len(TP), None, C.byref(h)) == -1
    assert b"range 0" in lib.bppp_last_error(gpu.h)
    rng[0].base = 3
    net = np.zeros(4, dtype=np.uint64)
    assert lib.bppp_rp_create_binary_seeded(gpu.h, 0, 0, C.cast(rng, C.c_void_p), 1, C.c_void_p(net.ctypes.data), TP, len(TP), None, C.byref(h)) == -1
    assert b"base must be 2" in lib.bppp_last_error(gpu.h)
