"""bppp_rp_excess_sign*, bppp_rp_excess_verify_each* and bppp_rp_excess_verify_batch* (excess signatures: a tally checked without revealing the
blinding sum) are declared in include/bppp.h, exported by the product library and typed in capi.py; the quad-walk hook is declared in
include/bppp_test.h and lives in the test library only; the nonce, challenge and weight messages, as rangeproof.excess_* restate them, are each
pinned against one vector put together by hand; rangeproof.excess_sign_host / excess_verify_host over the oracle backend accept what was signed
and nothing next to it, a forgery against a challenge that ignores X included; without a GPU, calls on a NULL handle fail with BPPP_ERR_ARG."""
import hashlib
import json
import os
import re
import subprocess

from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from rp_backends import OracleBackend
from test_rangeproof import EXAMPLES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
N, P = RP.N, RP.FIELD_P
NARGS = {"bppp_rp_excess_sign": 8, "bppp_rp_excess_sign_device": 8, "bppp_rp_excess_verify_each": 13, "bppp_rp_excess_verify_each_device": 13,
         "bppp_rp_excess_verify_batch": 15, "bppp_rp_excess_verify_batch_device": 16}
HOOK = "bppp_test_rp_excess_mul"
OK, MISMATCH, MALFORMED, NOT_CANONICAL, BAD_R, NO_KEY = 0, 1, 2, 3, 4, 5


def _header(name="bppp.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _limbs(v):
    """put by hand: limb i (64 bits, least significant first) big-endian"""
    return b"".join(((v >> (64 * i)) & (2**64 - 1)).to_bytes(8, "big") for i in range(4))


def _digest_mod_n(msg):
    d = hashlib.sha256(msg).digest()
    return sum(int.from_bytes(d[8 * i:8 * i + 8], "big") << (64 * i) for i in range(4)) % N


def test_the_six_symbols_are_declared_exported_and_bound():
    lib, tlib, hdr, thdr = capi.load_library(), capi.load_test_library(), _header(), _header("bppp_test.h")
    dyn = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in dyn.splitlines() if l.strip()}
    for name, nargs in NARGS.items():
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in exported, name
        assert name in capi.SYMBOLS and len(getattr(lib, name).argtypes) == nargs, name
    assert re.search(r"\b%s\s*\(" % HOOK, thdr) and hasattr(tlib, HOOK) and HOOK not in exported
    assert len(getattr(tlib, HOOK).argtypes) == 5 and getattr(tlib, HOOK)(None, 1, None, None, None) == ERR_ARG
    for cls in (RP.NativeRangeProofs, BRP.NativeBinaryRangeProofs):
        for method in ("excess_sign", "excess_sign_device", "excess_verify_each", "excess_verify_each_device", "excess_verify_batch", "excess_verify_batch_device"):
            assert callable(getattr(cls, method)), method
    assert "rpexcess.hip" in open(os.path.join(ROOT, "bulletproofspp_amd", "_build.py")).read()
    for name, value in (("SIG_BYTES", 65), ("OK", 0), ("NOT_CANONICAL", 1), ("ZERO", 2), ("NONCE", 3), ("BAD_R", 4), ("NO_KEY", 5)):
        assert re.search(r"#define\s+BPPP_RP_EXCESS_%s\s+%du?\b" % (name, value), hdr), name
        assert getattr(capi, "RP_EXCESS_" + name) == value


def test_null_handle_is_an_argument_error():
    lib = capi.load_library()
    for nsums in (0, 1):
        assert lib.bppp_rp_excess_sign(None, nsums, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_sign_device(None, nsums, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_verify_each(None, 1, None, nsums, None, None, 0, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_verify_each_device(None, 1, None, nsums, None, None, 0, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_verify_batch(None, 1, None, nsums, None, None, 0, None, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_verify_batch_device(None, 1, None, nsums, None, None, 0, None, None, None, None, 0, None, None, None, None) == ERR_ARG


TAG = b"excess tag"
MSG = bytes(range(100, 132))
AUX = bytes(range(200, 232))
X_PT = (5 + (7 << 64), P - 3)                  # the messages take any pair of coordinates: y > p - y, so the sign byte is 1
X33 = (5).to_bytes(8, "big") + (7).to_bytes(8, "big") + bytes(16) + b"\x01"


def test_excess_nonce_vector():
    """SHA-256 ("bppp/excess/nonce/v1" || tag) || put (e) || msg || aux: 128 bytes"""
    e = N - 1
    msg = hashlib.sha256(b"bppp/excess/nonce/v1" + b"excess tag").digest() + _limbs(N - 1) + MSG + AUX
    assert len(msg) == 128
    want = _digest_mod_n(msg)
    assert RP.excess_nonce(TAG, e, MSG, AUX) == want
    others = [RP.excess_nonce(TAG, e - 1, MSG, AUX), RP.excess_nonce(TAG, e, MSG[:-1] + b"\0", AUX), RP.excess_nonce(TAG, e, MSG, AUX[:-1] + b"\0"),
              RP.excess_nonce(TAG + b"x", e, MSG, AUX), RP.excess_nonce(b"", e, MSG, AUX)]
    assert want not in others and len(set(others)) == len(others)


def test_excess_challenge_vector():
    """SHA-256 ("bppp/excess/challenge/v1" || tag) || the 33 bytes of R || put (X.x) || sign (X) || msg: 130 bytes"""
    r33 = bytes(range(1, 33)) + b"\x00"
    msg = hashlib.sha256(b"bppp/excess/challenge/v1" + b"excess tag").digest() + r33 + X33 + MSG
    assert len(msg) == 130
    want = _digest_mod_n(msg)
    assert RP.excess_challenge(TAG, r33, X_PT, MSG) == want
    others = [RP.excess_challenge(TAG, r33[:32] + b"\x01", X_PT, MSG), RP.excess_challenge(TAG, r33, (X_PT[0] + 1, X_PT[1]), MSG),
              RP.excess_challenge(TAG, r33, (X_PT[0], 3), MSG), RP.excess_challenge(TAG, r33, X_PT, b"\0" + MSG[1:]), RP.excess_challenge(b"excess tah", r33, X_PT, MSG)]
    assert want not in others and len(set(others)) == len(others)


def test_excess_weight_vector():
    """seed || le64 (t) || sig[65] || put (X.x) || sign (X) || msg: 170 bytes; the signature holds s = n - 1, the position is >= 2^32"""
    seed = bytes(range(32))
    t = 0x0102030405060708
    sig = bytes(range(1, 33)) + b"\x01" + _limbs(N - 1)
    msg = seed + bytes([8, 7, 6, 5, 4, 3, 2, 1]) + sig + X33 + MSG
    assert len(msg) == 170 and len(sig) == 65
    want = _digest_mod_n(msg)
    assert want != 0 and RP.excess_weight(seed, t, sig, X_PT, MSG) == want
    assert RP.excess_weight(seed, t + 1, sig, X_PT, MSG) != want and RP.excess_weight(seed, t, sig[:64] + b"\0", X_PT, MSG) != want
    assert RP.excess_weight(seed, t, sig, (X_PT[0], 3), MSG) != want and RP.excess_weight(seed, t, sig, X_PT, MSG[:-1] + b"\0") != want
    assert RP.excess_weight(seed, t + 2**64, sig, X_PT, MSG) == want                  # the position is taken mod 2^64


def _setups(oracle_lib):
    be = OracleBackend(oracle_lib)
    typed = RP.setup_from_schema(be, json.load(open(os.path.join(EXAMPLES, "rec_test", "schema.json"))))
    binary = BRP.setup_from_schema(be, json.load(open(os.path.join(EXAMPLES, "bin_test", "schema.json"))))
    return be, typed, binary


def test_host_sign_then_verify(oracle_lib):
    ec = oracle_lib
    be, typed, binary = _setups(oracle_lib)
    for st in (typed, binary):
        is_typed = st is typed
        B = st.hs[1] if is_typed else st.hs[0]
        e, a, ty = 0x1234567890ABCDEF << 100, 77, (5 if is_typed else 0)
        status, sig, X = RP.excess_sign_host(be, st, e, MSG, AUX, TAG)
        assert status == 0 and len(sig) == 65 and X == ec.mul(e, B)
        assert RP.excess_sign_host(be, st, e, MSG, AUX, TAG) == (status, sig, X)      # deterministic in (e, msg, aux)
        assert RP.excess_sign_host(be, st, e, MSG, bytes(32), TAG)[1][:33] != sig[:33]
        S = ec.inner_product([(a, st.g), (e, B)] + ([(ty, st.hs[0])] if is_typed else []))
        claim = (a, ty)
        assert RP.excess_key_host(be, st, S, claim) == X
        assert RP.excess_verify_host(be, st, S, claim, MSG, sig, TAG) == OK
        s = sum(int.from_bytes(sig[33 + 8 * i:41 + 8 * i], "big") << (64 * i) for i in range(4))
        assert RP.excess_verify_host(be, st, S, claim, MSG, sig[:33] + _limbs((s + 1) % N), TAG) == MISMATCH
        assert RP.excess_verify_host(be, st, S, claim, MSG, sig[:33] + _limbs(N), TAG) == NOT_CANONICAL
        assert RP.excess_verify_host(be, st, S, claim, MSG[:-1] + b"\0", sig, TAG) == MISMATCH
        assert RP.excess_verify_host(be, st, S, (a + 1, ty), MSG, sig, TAG) == MISMATCH
        assert RP.excess_verify_host(be, st, S, claim, MSG, sig, TAG + b"2") == MISMATCH
        assert RP.excess_verify_host(be, st, S, claim, MSG, sig, b"") == MISMATCH
        assert RP.excess_verify_host(be, st, S, claim, MSG, sig[:32] + b"\x02" + sig[33:], TAG) == BAD_R
        assert RP.excess_verify_host(be, st, S, claim, MSG, sig[:32] + bytes([sig[32] ^ 1]) + sig[33:], TAG) == MISMATCH
        assert RP.excess_verify_host(be, st, ec.inner_product([(a, st.g)] + ([(ty, st.hs[0])] if is_typed else [])), claim, MSG, sig, TAG) == NO_KEY
        assert RP.excess_verify_host(be, st, S, claim, MSG, sig, TAG, malformed=True) == MALFORMED
        if is_typed:
            assert RP.excess_verify_host(be, st, S, (a, N), MSG, sig, TAG) == NOT_CANONICAL
            assert RP.excess_verify_host(be, st, S, (a, ty + 1), MSG, sig, TAG) == MISMATCH
        assert RP.excess_sign_host(be, st, 0, MSG, AUX, TAG) == (RP.EXCESS_ZERO, bytes(65), None)
        assert RP.excess_sign_host(be, st, N, MSG, AUX, TAG) == (RP.EXCESS_NOT_CANONICAL, bytes(65), None)


def test_forgery_against_a_challenge_without_x_fails_under_the_real_one(oracle_lib):
    """R = r B + d g; under c' = H (R, msg) the forger solves s B - c' X = R for the unbalanced X = (s - r) / c' B - d / c' g.  That X verifies
    under c' — the attack is real — and not under the challenge that hashes X."""
    ec = oracle_lib
    be, typed, _ = _setups(oracle_lib)
    st, B, g = typed, typed.hs[1], typed.g
    r, d, s = 0xABCDEF123456789, 3, 0x1111111111111111111
    R = ec.inner_product([(r, B), (d, g)])
    r33 = RP._point33(R)
    weak = RP.decode_field(hashlib.sha256(hashlib.sha256(b"bppp/excess/challenge/v1" + TAG).digest() + r33 + MSG).digest(), N)     # no X under the hash
    ci = RP.inv(weak)
    X = ec.inner_product([((s - r) * ci % N, B), ((-d) * ci % N, g)])
    assert ec.inner_product([(s, B), ((-weak) % N, X)]) == R                           # the forgery satisfies the weak equation
    # the validator's sum: claim amount 10, so S = X + 10 g hides  10 - d / c'  units of g
    S = ec.inner_product([(1, X), (10, g)])
    sig = r33 + _limbs(s)
    assert RP.excess_key_host(be, st, S, (10, 0)) == X
    assert RP.excess_verify_host(be, st, S, (10, 0), MSG, sig, TAG) == MISMATCH
