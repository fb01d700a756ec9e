"""bppp_rp_excess_part_nonces*, _part_aggregate*, _part_sign*, _part_verify* and _part_combine* (multi-party excess signatures: builders who each know a
part of the blinding sum) are declared in include/bppp.h, exported by the product library and typed in capi.py; BPPP_RP_EXCESS_NONCE_INFINITY matches
capi and rangeproof; calls on a NULL handle fail with BPPP_ERR_ARG without a GPU; rangeproof.excess_part_nonce and excess_nonce_coef are pinned against
hashlib over bytes put together by hand; over the oracle backend one, two and three parties sign on the host, and every verifier restatement accepts
the combined signature and nothing next to it."""
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
NARGS = {"bppp_rp_excess_part_nonces": 7, "bppp_rp_excess_part_nonces_device": 7, "bppp_rp_excess_part_aggregate": 9, "bppp_rp_excess_part_aggregate_device": 9,
         "bppp_rp_excess_part_sign": 9, "bppp_rp_excess_part_sign_device": 9, "bppp_rp_excess_part_verify": 10, "bppp_rp_excess_part_verify_device": 10,
         "bppp_rp_excess_part_combine": 11, "bppp_rp_excess_part_combine_device": 11}
OK, MISMATCH = 0, 1
TAG = b"excess part tag"
MSG = bytes(range(40, 72))
AUX = bytes(range(170, 202))


def _header(name="bppp.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _limbs(v):
    """put by hand: limb i (64 bits, least significant first) big-endian"""
    return b"".join(((v >> (64 * i)) & (2**64 - 1)).to_bytes(8, "big") for i in range(4))


def _value(b32):
    return sum(int.from_bytes(b32[8 * i:8 * i + 8], "big") << (64 * i) for i in range(4))


def test_the_ten_symbols_are_declared_exported_and_bound():
    lib, hdr = capi.load_library(), _header()
    dyn = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in dyn.splitlines() if l.strip()}
    for name, nargs in NARGS.items():
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in exported, name
        assert name in capi.SYMBOLS and len(getattr(lib, name).argtypes) == nargs, name
    for cls in (RP.NativeRangeProofs, BRP.NativeBinaryRangeProofs):
        for method in ("excess_part_nonces", "excess_part_aggregate", "excess_part_sign", "excess_part_verify", "excess_part_combine"):
            assert callable(getattr(cls, method)) and callable(getattr(cls, method + "_device")), method
    assert "rpexpart.hip" in open(os.path.join(ROOT, "bulletproofspp_amd", "_build.py")).read()
    for name, value in (("NONCE_INFINITY", 7), ("NO_AGGREGATE", 8), ("PUBNONCE_BYTES", 66), ("PARTIAL_BYTES", 32)):
        assert re.search(r"#define\s+BPPP_RP_EXCESS_%s\s+%du?\b" % (name, value), hdr), name
        assert getattr(capi, "RP_EXCESS_" + name) == value and getattr(RP, "EXCESS_" + name) == value
    thdr = _header("bppp_test.h")
    decl = re.search(r"\bbppp_test_rp_excess_mul2\s*\(([^;]*)\)\s*;", thdr)
    assert decl and len(decl.group(1).split(",")) == 7 and len(capi.load_test_library().bppp_test_rp_excess_mul2.argtypes) == 7


def test_null_handle_is_an_argument_error():
    lib = capi.load_library()
    for n in (0, 1):
        assert lib.bppp_rp_excess_part_nonces(None, n, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_part_nonces_device(None, n, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_part_aggregate(None, n, n, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_part_aggregate_device(None, n, n, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_part_sign(None, n, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_part_sign_device(None, n, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_part_verify(None, n, n, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_part_verify_device(None, n, n, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_part_combine(None, n, n, None, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_part_combine_device(None, n, n, None, None, None, None, None, None, None, None) == ERR_ARG


def test_the_two_hashes_against_hashlib():
    """every byte of the two new messages laid out by hand: 129 and 163 bytes"""
    e = 5 + (7 << 64) + (0x0102030405060708 << 192)
    e_bytes = (5).to_bytes(8, "big") + (7).to_bytes(8, "big") + bytes(8) + bytes([1, 2, 3, 4, 5, 6, 7, 8])
    dm = hashlib.sha256(b"bppp/excess/partnonce/v1" + TAG).digest()
    for j in (1, 2):
        text = dm + e_bytes + MSG + AUX + bytes([j])
        assert len(text) == 129
        assert RP.excess_part_nonce(TAG, e, MSG, AUX, j) == _value(hashlib.sha256(text).digest()) % N
    assert RP.excess_part_nonce(TAG, e, MSG, AUX, 1) != RP.excess_part_nonce(TAG, e, MSG, AUX, 2)
    assert RP.excess_part_nonce(TAG, e, MSG, AUX, 1) != RP.excess_nonce(TAG, e, MSG, AUX)          # another domain than the single signer's
    x = 9 + (11 << 128)
    x_bytes = (9).to_bytes(8, "big") + bytes(8) + (11).to_bytes(8, "big") + bytes(8)
    r1, r2 = bytes(range(33)), bytes(range(100, 133))
    db = hashlib.sha256(b"bppp/excess/noncecoef/v1" + TAG).digest()
    for y, sign in ((3, 0), (P - 3, 1)):
        text = db + r1 + r2 + x_bytes + bytes([sign]) + MSG
        assert len(text) == 163
        assert RP.excess_nonce_coef(TAG, r1, r2, (x, y), MSG) == _value(hashlib.sha256(text).digest()) % N


def _setups(oracle_lib):
    be = OracleBackend(oracle_lib)
    typed = RP.setup_from_schema(be, json.load(open(os.path.join(EXAMPLES, "rec_test", "schema.json"))))
    binary = BRP.setup_from_schema(be, json.load(open(os.path.join(EXAMPLES, "bin_test", "schema.json"))))
    return be, typed, binary


def test_parties_sign_on_the_host(oracle_lib):
    ec = oracle_lib
    be, typed, binary = _setups(oracle_lib)
    for st in (typed, binary):
        g, H0, B = RP._excess_bases(st)
        for nparties in (1, 2, 3):
            es = [(0x1234567890ABCDEF << (60 + 30 * i)) + 17 * i + 1 for i in range(nparties)]
            auxs = [hashlib.sha256(AUX + bytes([i])).digest() for i in range(nparties)]
            amounts = [1000 + i for i in range(nparties)]
            keys = [RP.excess_key33(ec.mul(e, B)) for e in es]
            round1 = [RP.excess_part_nonces_host(be, st, e, MSG, a, TAG) for e, a in zip(es, auxs)]
            assert [s for s, _ in round1] == [OK] * nparties
            nonces = [pn for _, pn in round1]
            for e, a, pn in zip(es, auxs, nonces):
                ks = [RP.excess_part_nonce(TAG, e, MSG, a, j) for j in (1, 2)]
                assert pn == b"".join(RP._point33(ec.mul(k, B)) for k in ks) and RP.excess_nonce(TAG, e, MSG, a) not in ks
            status, agg_nonce, agg_key = RP.excess_part_aggregate_host(be, st, nonces, keys)
            assert status == OK and RP.excess_lift33(agg_key) == ec.mul(sum(es) % N, B)
            round2 = [RP.excess_part_sign_host(be, st, e, MSG, a, agg_nonce, agg_key, TAG) for e, a in zip(es, auxs)]
            assert [s for s, _ in round2] == [OK] * nparties
            partials = [p for _, p in round2]
            assert RP.excess_part_verify_host(be, st, nonces, keys, partials, MSG, TAG) == ([OK] * nparties, OK)
            status, sig, key = RP.excess_part_combine_host(be, st, nonces, keys, partials, MSG, TAG)
            assert status == OK and key == agg_key and len(sig) == RP.EXCESS_SIG_BYTES
            # every verifier's restatement takes the 65 bytes as they are: under the stated key, and against the sum of the parties' commitments
            assert RP.excess_verify_key_host(be, st, agg_key, MSG, sig, TAG) == OK
            S = ec.inner_product([(a, g) for a in amounts] + [(e, B) for e in es])
            assert RP.excess_verify_host(be, st, S, (sum(amounts), 0), MSG, sig, TAG) == OK
            other = bytes(32)
            assert RP.excess_verify_key_host(be, st, agg_key, other, sig, TAG) == MISMATCH
            assert RP.excess_verify_host(be, st, S, (sum(amounts), 0), other, sig, TAG) == MISMATCH
            # one partial off by one: the signature no longer verifies and the check names that part alone
            for bad in range(nparties):
                forged = list(partials)
                forged[bad] = _limbs((_value(partials[bad]) + 1) % N)
                status, bad_sig, _ = RP.excess_part_combine_host(be, st, nonces, keys, forged, MSG, TAG)
                assert status == OK and RP.excess_verify_key_host(be, st, agg_key, MSG, bad_sig, TAG) == MISMATCH
                assert RP.excess_part_verify_host(be, st, nonces, keys, forged, MSG, TAG) == ([MISMATCH if i == bad else OK for i in range(nparties)], OK)
            # partials made for another message do not check under this one
            assert RP.excess_part_verify_host(be, st, nonces, keys, partials, other, TAG) == ([MISMATCH] * nparties, OK)


def test_host_verdicts(oracle_lib):
    ec = oracle_lib
    be, typed, _ = _setups(oracle_lib)
    _, _, B = RP._excess_bases(typed)
    e = 0xABCDEF << 90
    assert RP.excess_part_nonces_host(be, typed, 0, MSG, AUX, TAG) == (RP.EXCESS_ZERO, bytes(66))
    assert RP.excess_part_nonces_host(be, typed, N, MSG, AUX, TAG) == (RP.EXCESS_NOT_CANONICAL, bytes(66))
    _, pn = RP.excess_part_nonces_host(be, typed, e, MSG, AUX, TAG)
    key = RP.excess_key33(ec.mul(e, B))
    flip = lambda b33: b33[:32] + bytes([b33[32] ^ 1])
    refused = lambda st: (st, bytes(66), bytes(33))
    assert RP.excess_part_aggregate_host(be, typed, [pn], [key[:32] + b"\x02"]) == refused(RP.EXCESS_BAD_KEY)
    assert RP.excess_part_aggregate_host(be, typed, [pn[:65] + b"\x02"], [key[:32] + b"\x02"]) == refused(RP.EXCESS_BAD_KEY)
    assert RP.excess_part_aggregate_host(be, typed, [pn[:65] + b"\x02"], [key]) == refused(RP.EXCESS_BAD_R)
    assert RP.excess_part_aggregate_host(be, typed, [pn, pn], [key, flip(key)]) == refused(RP.EXCESS_NO_KEY)
    assert RP.excess_part_aggregate_host(be, typed, [pn, flip(pn[:33]) + pn[33:]], [key, key]) == refused(RP.EXCESS_NONCE_INFINITY)
    assert RP.excess_part_sign_host(be, typed, e, MSG, AUX, pn, key[:32] + b"\x02", TAG) == (RP.EXCESS_BAD_KEY, bytes(32))
    assert RP.excess_part_sign_host(be, typed, e, MSG, AUX, pn[:32] + b"\x02" + pn[33:], key, TAG) == (RP.EXCESS_BAD_R, bytes(32))
    assert RP.excess_part_sign_host(be, typed, 0, MSG, AUX, pn[:32] + b"\x02" + pn[33:], key, TAG) == (RP.EXCESS_ZERO, bytes(32))
    _, part = RP.excess_part_sign_host(be, typed, e, MSG, AUX, pn, key, TAG)
    assert RP.excess_part_verify_host(be, typed, [pn], [key], [_limbs(N)], MSG, TAG) == ([3], OK)
    assert RP.excess_part_verify_host(be, typed, [pn, pn], [key, flip(key)], [part, part], MSG, TAG) == ([RP.EXCESS_NO_KEY] * 2, RP.EXCESS_NO_KEY)
    # who misbehaved: the part that does not lift reads BAD_KEY or BAD_R, its honest cosigner NO_AGGREGATE
    assert RP.excess_part_verify_host(be, typed, [pn, pn], [key, key[:32] + b"\x02"], [part, part], MSG, TAG) == ([RP.EXCESS_NO_AGGREGATE, RP.EXCESS_BAD_KEY], RP.EXCESS_BAD_KEY)
    assert RP.excess_part_verify_host(be, typed, [pn[:65] + b"\x02", pn], [key, key], [part, part], MSG, TAG) == ([RP.EXCESS_BAD_R, RP.EXCESS_NO_AGGREGATE], RP.EXCESS_BAD_R)
    assert RP.excess_part_combine_host(be, typed, [pn, pn], [key, flip(key)], [part, part], MSG, TAG) == (RP.EXCESS_NO_KEY, bytes(65), bytes(33))
