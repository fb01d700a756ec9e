"""bppp_seed_candidate_x (host only, no GPU): x of candidate n of getPoints(seed) (app/Main.hs:68-72) against an inline restatement —
SHA-256 (seed <> decimal n), the digest read as four big-endian 64-bit words with the least significant first (Binary (Prime p),
src/Encoding.hs:75-79), mod p — and against rangeproof.decode_field.  The function runs the message building and hashing the candidate
kernel runs on the device (one BPPP_HD function, csrc/seedpoints.hip.h).  Seed lengths straddle the sizes at which the padding spills
into a second block (tail + digits + 9 > 64), n every digit count's edge up to twenty digits."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP

P = 2**256 - 2**32 - 977
SEED_LENS = [0, 11] + list(range(46, 57)) + [63, 64, 65, 119, 128, 4096]
NS = [0, 9, 10, 99, 100, 999, 1000, 2**32 - 1, 2**32, 10**19 - 1, 10**19, 2**64 - 1]


def _seed(length):
    return b"test points" if length == 11 else bytes((7 * i + length) & 0xFF for i in range(length))


def _restated_x(seed, n):
    d = hashlib.sha256(seed + str(n).encode()).digest()
    r = sum(int.from_bytes(d[8 * i:8 * i + 8], "big") << (64 * i) for i in range(4))
    return r % P


def _candidate_x(lib, seed, n):
    out = np.zeros(4, dtype=np.uint64)
    assert lib.bppp_seed_candidate_x(seed, len(seed), n, C.c_void_p(out.ctypes.data)) == 0
    return capi.limbs_to_int(out)


@pytest.mark.parametrize("length", SEED_LENS)
def test_candidate_x_matches_the_restatement(length):
    lib = capi.load_library()
    seed = _seed(length)
    for n in NS:
        want = _restated_x(seed, n)
        assert want == RP.decode_field(hashlib.sha256(seed + str(n).encode()).digest(), P)
        assert _candidate_x(lib, seed, n) == want, (length, n)


def test_null_seed_is_the_empty_seed():
    lib = capi.load_library()
    out = np.zeros(4, dtype=np.uint64)
    assert lib.bppp_seed_candidate_x(None, 0, 5, C.c_void_p(out.ctypes.data)) == 0
    assert capi.limbs_to_int(out) == _restated_x(b"", 5)


def test_argument_errors():
    lib = capi.load_library()
    out = np.zeros(4, dtype=np.uint64)
    assert lib.bppp_seed_candidate_x(b"s" * 4097, 4097, 0, C.c_void_p(out.ctypes.data)) == -1
    assert lib.bppp_seed_candidate_x(None, 3, 0, C.c_void_p(out.ctypes.data)) == -1
    assert lib.bppp_seed_candidate_x(b"abc", 3, 0, None) == -1
    assert not out.any()
