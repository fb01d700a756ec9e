"""bppp_rp_tally_each*, bppp_rp_tally_batch* and bppp_rp_tally_claims* (signed sums of commitments against claimed openings) are declared in
include/bppp.h, exported by the product library and typed in capi.py; their three threshold hooks are declared in include/bppp_test.h and live
in the test library only; the weight message of bppp_rp_tally_batch, as rangeproof.tally_weight restates it, is pinned against one vector put
together by hand; rangeproof.tally_claims_host equals plain integer arithmetic mod n; without a GPU, calls on a NULL handle fail with
BPPP_ERR_ARG instead of crashing."""
import hashlib
import os
import random
import re
import subprocess

from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NARGS = {"bppp_rp_tally_each": 12, "bppp_rp_tally_each_device": 12, "bppp_rp_tally_batch": 14, "bppp_rp_tally_batch_device": 15, "bppp_rp_tally_claims": 12,
         "bppp_rp_tally_claims_device": 12}
HOOKS = ["bppp_test_rp_set_tally_short_max", "bppp_test_rp_set_tally_piece", "bppp_test_rp_set_tally_chunk"]


def _header(name="bppp.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_nine_symbols_are_declared_exported_and_bound():
    lib, tlib, hdr, thdr = capi.load_library(), capi.load_test_library(), _header(), _header("bppp_test.h")
    dyn = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in dyn.splitlines() if l.strip()}
    for name, nargs in NARGS.items():
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in exported, name
        assert name in capi.SYMBOLS and len(getattr(lib, name).argtypes) == nargs, name
    for name in HOOKS:
        assert re.search(r"\b%s\s*\(" % name, thdr) and hasattr(tlib, name) and name not in exported, name
        assert getattr(tlib, name)(None, 4) == ERR_ARG
    from bulletproofspp_amd.rangeproof_binary import NativeBinaryRangeProofs
    for cls in (RP.NativeRangeProofs, NativeBinaryRangeProofs):
        for method in ("tally_each", "tally_each_device", "tally_batch", "tally_batch_device", "tally_claims", "tally_claims_device"):
            assert callable(getattr(cls, method)), method
    assert "rptally.hip" in open(os.path.join(ROOT, "bulletproofspp_amd", "_build.py")).read()


def test_tally_weight_vector():
    """seed || le64(t) || put(a) || put(ty) || put(e), put = four 64-bit limbs least significant first, each big-endian; the digest read the
    same way and reduced mod n"""
    seed = bytes(range(32))
    t = 0x0102030405060708
    a, ty, e = 5, 2**64 + 7, RP.N - 1
    msg = seed + bytes([8, 7, 6, 5, 4, 3, 2, 1])
    msg += (5).to_bytes(8, "big") + bytes(24)                                         # a: limb 0 = 5
    msg += (7).to_bytes(8, "big") + (1).to_bytes(8, "big") + bytes(16)                # ty: limb 0 = 7, limb 1 = 1
    msg += b"".join((((RP.N - 1) >> (64 * i)) & (2**64 - 1)).to_bytes(8, "big") for i in range(4))
    assert len(msg) == 136
    d = hashlib.sha256(msg).digest()
    want = sum(int.from_bytes(d[8 * i:8 * i + 8], "big") << (64 * i) for i in range(4)) % RP.N
    assert want != 0 and RP.tally_weight(seed, t, a, ty, e) == want
    assert RP.tally_weight(seed, t + 1, a, ty, e) != want and RP.tally_weight(seed, t, a, ty, e - 1) != want
    assert RP.tally_weight(seed, t + 2**64, a, ty, e) == want                          # the position is taken mod 2^64


def test_tally_claims_host_is_integer_arithmetic_mod_n():
    rng = random.Random(11)
    N = RP.N
    triples = [(rng.randrange(-2**70, 2**70), rng.randrange(N), rng.randrange(N)) for _ in range(12)]
    triples[3] = (-(2**255) + 5, 0, N - 1)                                             # the most negative amounts, the largest blinding
    triples[4] = (-1, N - 1, N - 1)
    sums = [[], [(3, False)], [(3, True)], [(3, False), (3, False), (4, True)], [(j, bool(j & 1)) for j in range(12)], [(4, True)] * 5]
    sum_start, entries = [0], []
    for s in sums:
        entries += [RP.tally_entry(j, sub) for j, sub in s]
        sum_start.append(len(entries))
    assert entries[1] == 3 | 2**31 and RP.tally_entry(5) == 5
    got = RP.tally_claims_host(triples, sum_start, entries)
    for s, claim in zip(sums, got):
        for k in range(3):
            assert claim[k] == sum((-1 if sub else 1) * triples[j][k] for j, sub in s) % N
    assert got[0] == (0, 0, 0) and got[2] == ((2**255 - 5) % N, 0, 1)
    # the word an amount travels as: its residue below 2^255, else the residue - n in two's complement — read back, the same residue
    for a in (0, 5, -5, N - 1, 2**255 - 1, 2**255, -(2**255) + 5, 3 * N + 2):
        w = RP.tally_amount_word(a)
        assert 0 <= w < 2**256 and (w - 2**256 if w >= 2**255 else w) % N == a % N


def test_null_handle_is_an_argument_error():
    lib = capi.load_library()
    for nsums in (0, 1):
        assert lib.bppp_rp_tally_each(None, 1, None, nsums, None, None, 0, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_tally_each_device(None, 1, None, nsums, None, None, 0, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_tally_batch(None, 1, None, nsums, None, None, 0, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_tally_batch_device(None, 1, None, nsums, None, None, 0, None, None, None, 0, None, None, None, None) == ERR_ARG
        assert lib.bppp_rp_tally_claims(None, 1, None, None, None, nsums, None, None, 0, None, None, None) == ERR_ARG
        assert lib.bppp_rp_tally_claims_device(None, 1, None, None, None, nsums, None, None, 0, None, None, None) == ERR_ARG
