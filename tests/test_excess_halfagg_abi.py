"""bppp_rp_excess_halfagg*, bppp_rp_excess_halfagg_verify* and bppp_rp_verify_block_agg* (half-aggregate excess signatures: 33 bytes a kernel and one
scalar) are declared in include/bppp.h, exported by the product library and typed in capi.py; calls on a NULL handle fail with BPPP_ERR_ARG without a
GPU; rangeproof.excess_halfagg_root is pinned against trees written out by hand; the coefficients depend on the order of the triples and on n; over
the oracle backend the host aggregate of what excess_sign_host signed verifies under excess_halfagg_verify_host and nothing next to it does; and two
signatures altered so that their plain sum is unchanged are refused, although the unweighted equation would still hold."""
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
NARGS = {"bppp_rp_excess_halfagg": 7, "bppp_rp_excess_halfagg_device": 7, "bppp_rp_excess_halfagg_verify": 8, "bppp_rp_excess_halfagg_verify_device": 8,
         "bppp_rp_verify_block_agg": 7, "bppp_rp_verify_block_agg_device": 7}
OK, MISMATCH, NOT_CANONICAL, BAD_R, BAD_KEY = 0, 1, 3, 4, 6
TAG = b"halfagg tag"
AUX = bytes(range(150, 182))
H = lambda b: hashlib.sha256(b).digest()


def _header(name="bppp.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _limbs(v):
    """put by hand: limb i (64 bits, least significant first) big-endian"""
    return b"".join(((v >> (64 * i)) & (2**64 - 1)).to_bytes(8, "big") for i in range(4))


def _s_of(b32):
    return sum(int.from_bytes(b32[8 * i:8 * i + 8], "big") << (64 * i) for i in range(4))


def test_the_six_symbols_are_declared_exported_and_bound():
    lib, hdr = capi.load_library(), _header()
    dyn = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in dyn.splitlines() if l.strip()}
    for name, nargs in NARGS.items():
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in exported, name
        assert name in capi.SYMBOLS and len(getattr(lib, name).argtypes) == nargs, name
    for cls in (RP.NativeRangeProofs, BRP.NativeBinaryRangeProofs):
        for method in ("excess_halfagg", "excess_halfagg_verify", "verify_block_agg"):
            assert callable(getattr(cls, method)) and callable(getattr(cls, method + "_device")), method
    assert "rpexagg.hip" in open(os.path.join(ROOT, "bulletproofspp_amd", "_build.py")).read()
    assert re.search(r"#define\s+BPPP_RP_EXCESS_AGG_BYTES\(n\)\s+\(33 \* \(size_t\)\(n\) \+ 32\)", hdr)
    assert [RP.EXCESS_AGG_BYTES(n) for n in (1, 2, 100)] == [65, 98, 3332]


def test_null_handle_is_an_argument_error():
    lib = capi.load_library()
    blk = capi.RpBlock()
    for n in (0, 1):
        blk.nkeys = n
        assert lib.bppp_rp_excess_halfagg(None, n, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_halfagg_device(None, n, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_halfagg_verify(None, n, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_excess_halfagg_verify_device(None, n, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_verify_block_agg(None, blk, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_verify_block_agg_device(None, blk, None, None, None, None, None) == ERR_ARG


def test_the_root_against_trees_written_out_by_hand():
    dn = H(b"bppp/excess/halfagg/node/v1" + TAG)
    node = lambda a, b: H(dn + a + b)
    L = [H(b"leaf %d" % i) for i in range(8)]
    root = lambda n: RP.excess_halfagg_root(TAG, L[:n])
    assert root(1) == L[0]                                                  # the leaf itself
    assert root(2) == node(L[0], L[1])
    assert root(3) == node(node(L[0], L[1]), L[2])                          # the odd node moves up from level 0
    assert root(5) == node(node(node(L[0], L[1]), node(L[2], L[3])), L[4])   # ... from level 0 and again from level 1
    assert root(8) == node(node(node(L[0], L[1]), node(L[2], L[3])), node(node(L[4], L[5]), node(L[6], L[7])))
    assert len({root(n) for n in (1, 2, 3, 5, 8)}) == 5
    # the leaf and the coefficient, byte for byte
    x = 5 + (7 << 16)                                                       # x + p still fits 256 bits
    key, r33, msg = _limbs(x + P) + b"\x01", bytes(range(33)), bytes(range(40, 72))        # an x that is not reduced: the leaf takes x mod p
    assert RP.excess_halfagg_leaf(TAG, r33, key, msg) == H(H(b"bppp/excess/halfagg/leaf/v1" + TAG) + r33 + _limbs(x) + b"\x01" + msg)
    z = _s_of(H(H(b"bppp/excess/halfagg/coef/v1" + TAG) + L[0] + (3).to_bytes(8, "little") + (2).to_bytes(8, "little"))) % N or 1
    assert RP.excess_halfagg_coef(TAG, L[0], 3, 2) == z
    s32 = _limbs(12345)
    assert RP.block_agg_weight(L[1], 3, L[0], s32) == (_s_of(H(L[1] + (3).to_bytes(8, "little") + L[0] + s32)) % N or 1)


def test_every_coefficient_depends_on_the_order_and_on_n():
    L = [H(b"triple %d" % i) for i in range(6)]
    coefs = lambda leaves, n: [RP.excess_halfagg_coef(TAG, RP.excess_halfagg_root(TAG, leaves), n, i) for i in range(len(leaves))]
    base = coefs(L, 6)
    swapped = coefs([L[1], L[0]] + L[2:], 6)
    assert all(a != b for a, b in zip(base, swapped))
    root = RP.excess_halfagg_root(TAG, L)
    other_n = [RP.excess_halfagg_coef(TAG, root, 7, i) for i in range(6)]                     # the same leaves and root under another n
    assert all(a != b for a, b in zip(base, other_n))
    assert all(a != b for a, b in zip(base, coefs(L[:5], 5) + [None]))


def _setups(oracle_lib):
    be = OracleBackend(oracle_lib)
    typed = RP.setup_from_schema(be, json.load(open(os.path.join(EXAMPLES, "rec_test", "schema.json"))))
    binary = BRP.setup_from_schema(be, json.load(open(os.path.join(EXAMPLES, "bin_test", "schema.json"))))
    return be, typed, binary


def _no_point_x(ec):
    x = 0
    while ec.lift_x(x) is not None:
        x += 1
    return x


def _job(be, st, n):
    es = [(0x1234567890ABCDEF << (60 + 7 * i)) % N for i in range(n)]
    msgs = [H(b"kernel %d" % i) for i in range(n)]
    out = [RP.excess_sign_host(be, st, e, m, AUX, TAG) for e, m in zip(es, msgs)]
    assert all(o[0] == 0 for o in out)
    return [RP.excess_key33(o[2]) for o in out], msgs, [o[1] for o in out]


def test_host_aggregate_verifies_and_nothing_next_to_it(oracle_lib):
    ec = oracle_lib
    be, typed, binary = _setups(oracle_lib)
    bx = _no_point_x(ec)
    for st in (typed, binary):
        for n in (1, 3):
            keys, msgs, sigs = _job(be, st, n)
            assert all(RP.excess_verify_key_host(be, st, k, m, g, TAG) == OK for k, m, g in zip(keys, msgs, sigs))
            agg = RP.excess_halfagg_host(TAG, keys, msgs, sigs)
            assert len(agg) == RP.EXCESS_AGG_BYTES(n) and agg[:33 * n] == b"".join(g[:33] for g in sigs)
            verify = lambda k=keys, m=msgs, a=agg, t=TAG: RP.excess_halfagg_verify_host(be, st, k, m, a, t)
            assert verify() == (True, [OK] * n, None)
            last = n - 1
            for changed in (verify(m=msgs[:last] + [msgs[last][:-1] + b"\0"]), verify(k=keys[:last] + [keys[last][:32] + bytes([keys[last][32] ^ 1])]),
                            verify(a=agg[:32] + bytes([agg[32] ^ 1]) + agg[33:]), verify(a=agg[:33 * n] + _limbs((_s_of(agg[33 * n:]) + 1) % N)), verify(t=TAG + b"2")):
                assert changed[0] is False and changed[1] == [MISMATCH] * n and changed[2] is not None
            assert verify(a=agg[:33 * n] + _limbs(N))[:2] == (False, [NOT_CANONICAL] * n)
            assert verify(a=agg[:33 * n] + _limbs(2**256 - 1))[:2] == (False, [NOT_CANONICAL] * n)
            st_badkey = verify(k=[keys[0][:32] + b"\x02"] + keys[1:])
            assert st_badkey[0] is False and st_badkey[1][0] == BAD_KEY and set(st_badkey[1][1:]) <= {MISMATCH}
            st_badr = verify(a=_limbs(bx) + agg[32:])
            assert st_badr[0] is False and st_badr[1][0] == BAD_R
            if n > 1:                                                       # two triples swapped, the aggregate as it was
                assert verify(k=[keys[1], keys[0]] + keys[2:], m=[msgs[1], msgs[0]] + msgs[2:])[0] is False
            # the aggregator's refusals: all zero bytes
            for bad_sigs, bad_keys in (([sigs[0][:33] + _limbs(N)] + sigs[1:], keys), ([sigs[0][:32] + b"\x02" + sigs[0][33:]] + sigs[1:], keys),
                                       (sigs, [_limbs(bx) + keys[0][32:]] + keys[1:])):
                assert RP.excess_halfagg_host(TAG, bad_keys, msgs, bad_sigs) == bytes(RP.EXCESS_AGG_BYTES(n))
    assert RP.excess_halfagg_host(TAG, [], [], []) == b"" and RP.excess_halfagg_verify_host(be, typed, [], [], b"", TAG) == (True, [], None)


def test_a_cancelling_pair_is_refused(oracle_lib):
    """s_1 + 1 and s_2 - 1: the plain sum of the responses is unchanged, so the UNWEIGHTED equation  (sum s) B - sum (c_i X_i + R_i) = identity  still
    holds — shown here on integers and on the curve — while each signature alone is wrong; the coefficients drawn from the tree refuse the pair"""
    ec = oracle_lib
    be, typed, binary = _setups(oracle_lib)
    for st in (typed, binary):
        _, _, B = RP._excess_bases(st)
        keys, msgs, sigs = _job(be, st, 2)
        s = [_s_of(g[33:]) for g in sigs]
        bent = [sigs[0][:33] + _limbs((s[0] + 1) % N), sigs[1][:33] + _limbs((s[1] - 1) % N)]
        assert (s[0] + 1 + s[1] - 1) % N == (s[0] + s[1]) % N
        Xs, Rs = [RP.excess_lift33(k) for k in keys], [RP.excess_lift33(g[:33]) for g in sigs]
        cs = [RP.excess_challenge(TAG, g[:33], X, m) for g, X, m in zip(sigs, Xs, msgs)]
        unweighted = lambda ss: ec.inner_product([(sum(ss) % N, B)] + [((N - c) % N, X) for c, X in zip(cs, Xs)] + [(N - 1, R) for R in Rs])
        assert unweighted(s) is None and unweighted([s[0] + 1, s[1] - 1]) is None
        assert [RP.excess_verify_key_host(be, st, k, m, g, TAG) for k, m, g in zip(keys, msgs, bent)] == [MISMATCH, MISMATCH]
        agg = RP.excess_halfagg_host(TAG, keys, msgs, bent)                 # the aggregator does not evaluate the equation: it aggregates them
        assert agg != bytes(98) and agg[:66] == sigs[0][:33] + sigs[1][:33]
        accept, status, point = RP.excess_halfagg_verify_host(be, st, keys, msgs, agg, TAG)
        assert accept is False and status == [MISMATCH, MISMATCH] and point is not None
        # what is left is (z_1 - z_2) B: the coefficients differ, so it cannot vanish
        root = RP.excess_halfagg_root(TAG, [RP.excess_halfagg_leaf(TAG, g[:33], k, m) for g, k, m in zip(sigs, keys, msgs)])
        z = [RP.excess_halfagg_coef(TAG, root, 2, i) for i in range(2)]
        assert z[0] != z[1] and point == ec.mul((z[0] - z[1]) % N, B)
