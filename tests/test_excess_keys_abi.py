"""bppp_rp_excess_keys*, bppp_rp_excess_verify_keys_each*, bppp_rp_excess_verify_keys_batch*, bppp_rp_excess_sums_each* and bppp_rp_excess_sums_batch*
(the excess stated as a 33-byte key: signatures checked with no pool, sums checked after cut-through) are declared in include/bppp.h, exported by
the product library and typed in capi.py; BPPP_RP_EXCESS_BAD_KEY matches capi; calls on a NULL handle fail with BPPP_ERR_ARG without a GPU;
rangeproof.excess_key33 is pinned against one vector put together by hand; rangeproof.excess_verify_key_host over the oracle backend accepts what
excess_sign_host signed under the stated key and nothing next to it; rangeproof.excess_sums_host accepts a block after cut-through and refuses it
with a key left out or a fee changed."""
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
NARGS = {"bppp_rp_excess_keys": 5, "bppp_rp_excess_keys_device": 5, "bppp_rp_excess_verify_keys_each": 6, "bppp_rp_excess_verify_keys_each_device": 6,
         "bppp_rp_excess_verify_keys_batch": 9, "bppp_rp_excess_verify_keys_batch_device": 10, "bppp_rp_excess_sums_each": 15, "bppp_rp_excess_sums_each_device": 15,
         "bppp_rp_excess_sums_batch": 17, "bppp_rp_excess_sums_batch_device": 18}
OK, MISMATCH, MALFORMED, NOT_CANONICAL, BAD_R, NO_KEY, BAD_KEY = 0, 1, 2, 3, 4, 5, 6
TAG = b"excess keys tag"
MSG = bytes(range(60, 92))
AUX = bytes(range(150, 182))


def _header(name="bppp.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _limbs(v):
    """put by hand: limb i (64 bits, least significant first) big-endian"""
    return b"".join(((v >> (64 * i)) & (2**64 - 1)).to_bytes(8, "big") for i in range(4))


def _no_point_x(ec):
    """as test_gpu_commit_open finds it: the first x whose x^3 + 7 is no square"""
    x = 0
    while ec.lift_x(x) is not None:
        x += 1
    return x


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
        for method in ("excess_keys", "excess_verify_keys_each", "excess_verify_keys_batch", "excess_sums_each", "excess_sums_batch"):
            assert callable(getattr(cls, method)) and callable(getattr(cls, method + "_device")), method
    assert "rpexkeys.hip" in open(os.path.join(ROOT, "bulletproofspp_amd", "_build.py")).read()
    for name, value in (("BAD_KEY", 6), ("KEY_BYTES", 33)):
        assert re.search(r"#define\s+BPPP_RP_EXCESS_%s\s+%du?\b" % (name, value), hdr), name
        assert getattr(capi, "RP_EXCESS_" + name) == value
    assert RP.EXCESS_BAD_KEY == 6 and RP.EXCESS_KEY_BYTES == 33


def test_null_handle_is_an_argument_error():
    lib = capi.load_library()
    for n in (0, 1):
        assert lib.bppp_rp_excess_keys(None, n, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_keys_device(None, n, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_verify_keys_each(None, n, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_verify_keys_each_device(None, n, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_verify_keys_batch(None, n, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_verify_keys_batch_device(None, n, None, None, None, 0, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_sums_each(None, 1, None, n, None, None, 0, None, None, None, n, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_sums_each_device(None, 1, None, n, None, None, 0, None, None, None, n, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_sums_batch(None, 1, None, n, None, None, 0, None, None, None, n, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_sums_batch_device(None, 1, None, n, None, None, 0, None, None, None, n, None, None, 0, None, None, None, None) == ERR_ARG


def test_excess_key33_vector():
    """put (x): limb i big-endian, least significant limb first; then 1 when y > p - y"""
    x = 5 + (7 << 64) + (0x0102030405060708 << 192)
    head = (5).to_bytes(8, "big") + (7).to_bytes(8, "big") + bytes(8) + bytes([1, 2, 3, 4, 5, 6, 7, 8])
    assert RP.excess_key33((x, P - 3)) == head + b"\x01" and RP.excess_key33((x, 3)) == head + b"\x00"
    assert RP.excess_key33((x, (P - 1) // 2)) == head + b"\x00" and RP.excess_key33((x, (P + 1) // 2)) == head + b"\x01"
    assert len(RP.excess_key33((x, 3))) == RP.EXCESS_KEY_BYTES


def _setups(oracle_lib):
    be = OracleBackend(oracle_lib)
    typed = RP.setup_from_schema(be, json.load(open(os.path.join(EXAMPLES, "rec_test", "schema.json"))))
    binary = BRP.setup_from_schema(be, json.load(open(os.path.join(EXAMPLES, "bin_test", "schema.json"))))
    return be, typed, binary


def _s_of(sig):
    return sum(int.from_bytes(sig[33 + 8 * i:41 + 8 * i], "big") << (64 * i) for i in range(4))


def test_host_sign_then_verify_under_the_stated_key(oracle_lib):
    ec = oracle_lib
    be, typed, binary = _setups(oracle_lib)
    bx = _no_point_x(ec)
    for st in (typed, binary):
        B = st.hs[1] if st is typed else st.hs[0]
        e, e2 = 0x1234567890ABCDEF << 100, 0xFEDCBA987 << 150
        status, sig, X = RP.excess_sign_host(be, st, e, MSG, AUX, TAG)
        assert status == 0 and X == ec.mul(e, B)
        key, other = RP.excess_key33(X), RP.excess_key33(ec.mul(e2, B))
        assert RP.excess_lift33(key) == X and len(key) == 33
        verify = lambda k=key, m=MSG, g=sig, t=TAG: RP.excess_verify_key_host(be, st, k, m, g, t)
        assert verify() == OK
        assert verify(g=sig[:33] + _limbs((_s_of(sig) + 1) % N)) == MISMATCH
        assert verify(m=MSG[:-1] + b"\0") == MISMATCH
        assert verify(t=TAG + b"2") == MISMATCH
        assert verify(k=key[:32] + bytes([key[32] ^ 1])) == MISMATCH                   # the key's sign flipped: the other point on the same x
        assert verify(k=other) == MISMATCH                                             # a different sum's key
        assert verify(g=sig[:33] + _limbs(N)) == NOT_CANONICAL
        assert verify(g=sig[:32] + b"\x02" + sig[33:]) == BAD_R
        assert verify(g=_limbs(bx) + sig[32:]) == BAD_R
        assert verify(k=key[:32] + b"\x02") == BAD_KEY
        assert verify(k=_limbs(bx) + key[32:]) == BAD_KEY
        assert verify(k=key[:32] + b"\x02", g=sig[:32] + b"\x02" + _limbs(N)) == BAD_KEY   # the key is judged first
        assert verify(g=sig[:32] + b"\x02" + _limbs(N)) == NOT_CANONICAL                   # then s, then R
        # an x that is not reduced names the point of x mod p, and the hashes take that point's canonical bytes: the same verdict
        if X[0] + P < 2**256:
            assert verify(k=_limbs(X[0] + P) + key[32:]) == OK
        # the derived-key path and the stated-key path agree on one signature
        S = ec.inner_product([(77, st.g), (e, B)])
        assert RP.excess_verify_host(be, st, S, (77, 0), MSG, sig, TAG) == OK


def _cut_through(ec, st, typed):
    """Transaction 1 spends A into B and C with fee f1, transaction 2 spends B into D with fee f2 (outputs minus inputs: the amount of a sum is minus
    its fee).  Each builder splits its blinding sum e into a revealed offset o and a signing key k = e - o.  Returns the witnesses, the block's
    sum - A + C + D with B gone, its claim and the two keys."""
    g, H0, Bg = RP._excess_bases(st)
    f1, f2 = 500, 70
    amounts = {"A": 1000000, "B": 400000, "C": 1000000 - 400000 - f1, "D": 400000 - f2}
    ty = 9 if typed else 0
    blind = {n: int.from_bytes(n.encode() * 31, "big") % N for n in "ABCD"}
    point = {n: ec.inner_product([(amounts[n], g), (blind[n], Bg)] + ([(ty, H0)] if typed else [])) for n in "ABCD"}
    e1, e2 = (blind["B"] + blind["C"] - blind["A"]) % N, (blind["D"] - blind["B"]) % N
    o1, o2 = 0x1111111111111111111111 % N, 0x2222222222222222222222222 % N
    k1, k2 = (e1 - o1) % N, (e2 - o2) % N
    S = ec.inner_product([(N - 1, point["A"]), (1, point["C"]), (1, point["D"])])
    a, t = (-(f1 + f2)) % N, (ty + ty - ty) % N
    claim = (a, t, (o1 + o2) % N) if typed else (a, (o1 + o2) % N)
    return S, claim, (k1, k2), (f1, f2)


def test_cut_through_on_the_host(oracle_lib):
    ec = oracle_lib
    be, typed, binary = _setups(oracle_lib)
    for st in (typed, binary):
        is_typed = st is typed
        Bg = st.hs[1] if is_typed else st.hs[0]
        S, claim, (k1, k2), _ = _cut_through(ec, st, is_typed)
        keys = [RP.excess_key33(ec.mul(k, Bg)) for k in (k1, k2)]
        msgs = [MSG, MSG[::-1]]
        sigs = [RP.excess_sign_host(be, st, k, m, AUX, TAG)[1] for k, m in zip((k1, k2), msgs)]
        assert [RP.excess_verify_key_host(be, st, k, m, g, TAG) for k, m, g in zip(keys, msgs, sigs)] == [OK, OK]
        assert RP.excess_verify_key_host(be, st, keys[1], msgs[0], sigs[0], TAG) == MISMATCH      # a signature under the other transaction's key
        verdict, rest = RP.excess_sums_host(be, st, S, claim, keys)
        assert verdict == OK and rest == ec.inner_product([(1, S), (N - 1, ec.mul(k1, Bg)), (N - 1, ec.mul(k2, Bg))])
        assert RP.excess_sums_host(be, st, S, claim, keys[::-1])[0] == OK
        assert RP.excess_sums_host(be, st, S, claim, keys[:1])[0] == MISMATCH                     # a key left out
        assert RP.excess_sums_host(be, st, S, ((claim[0] + 1) % N,) + tuple(claim[1:]), keys)[0] == MISMATCH     # a fee off by one
        assert RP.excess_sums_host(be, st, S, tuple(claim[:-1]) + ((claim[-1] + 1) % N,), keys)[0] == MISMATCH   # another offset
        assert RP.excess_sums_host(be, st, S, tuple(claim[:-1]) + (N,), keys)[0] == NOT_CANONICAL
        assert RP.excess_sums_host(be, st, S, claim, keys + [keys[0][:32] + b"\x02"]) == (BAD_KEY, None)
        assert RP.excess_sums_host(be, st, S, claim, keys + [keys[0][:32] + b"\x02"], malformed=True) == (MALFORMED, None)
        assert RP.excess_sums_host(be, st, S, claim, keys + [keys[0]])[0] == MISMATCH              # a duplicate is subtracted twice, not rejected
        # no keys: a tally with the offset as the claimed blinding
        e = (k1 + k2 + claim[-1]) % N
        assert RP.excess_sums_host(be, st, S, tuple(claim[:-1]) + (e,), []) == (OK, S)
