"""bppp_rp_verify_block_agg*: bppp_rp_verify_block with the half-aggregate of the kernel signatures in their place, still one call and ONE MSM.

The blocks are test_gpu_block's (9 pool rows, the first 5 proven), cut to two sums: sums 0 and 1 with their 3 keys, and sums 0 and 2 with the 1 key of
sum 0.  The reference side of the combined point is  V + rho_A K' + S:  V and S from bppp_rp_verify_bound and bppp_rp_excess_sums_batch under
rangeproof.block_seeds (seed), K' the point of bppp_rp_excess_halfagg_verify (itself checked against the oracle in test_gpu_excess_halfagg), rho_A
from rangeproof.block_agg_weight over the root that hashlib gives, the scalar multiple and the additions by the CPU oracle."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from test_gpu_block import AUX, NPROOFS, ROWS, SEED, SEED2, TAG, Block, _block, _counts, _parts, _sum3, _tamper_proof, handles      # noqa: F401 (handles: a fixture)

pytestmark = pytest.mark.gpu

N = O.N
NAMES = ["rec_test", "bin_test"]
CUTS = {3: (0, 1), 1: (0, 2)}                            # nkeys -> the two sums kept
VALID, INVALID = 0, 1
OK, MISMATCH, NOT_CANONICAL, BAD_R, BAD_KEY = 0, 1, 3, 4, 6


def _cut(handles, name, nkeys):
    """test_gpu_block's block with two of its sums, and the half-aggregate of the keys that are left (restated on the host)"""
    full = _block(handles, name)
    ss, en, ks, claims, rows = [0], [], [0], [], []
    for t in CUTS[nkeys]:
        en += full.en[full.ss[t]:full.ss[t + 1]]
        ss.append(len(en))
        rows += list(range(full.ks[t], full.ks[t + 1]))
        ks.append(len(rows))
        claims.append(full.claims[t])
    pick = lambda xs: [xs[k] for k in rows]
    blk = Block(coms=list(full.coms), proofs=list(full.proofs), ss=ss, en=en, claims=claims, ks=ks, keys=pick(full.keys), msgs=pick(full.msgs), sigs=pick(full.sigs),
                bindings=list(full.bindings))
    assert len(blk.keys) == nkeys
    return blk, RP.excess_halfagg_host(TAG, blk.keys, blk.msgs, blk.sigs)


def _args(blk, agg):
    return (blk.coms, blk.proofs, blk.ss, blk.en, blk.claims, blk.ks, blk.keys, blk.msgs, agg)


def _both(nat, blk, agg, seed=SEED):
    host = nat.verify_block_agg(*_args(blk, agg), bindings=blk.bindings, seed=seed, want_status=True, want_point=True)
    assert nat.verify_block_agg_device(*_args(blk, agg), bindings=blk.bindings, seed=seed, want_status=True, want_point=True) == host
    return host


def _with_s(agg, s):
    return agg[:-32] + RP._put(s)


def _s_agg(agg):
    return sum(int.from_bytes(agg[len(agg) - 32 + 8 * i:len(agg) - 24 + 8 * i], "big") << (64 * i) for i in range(4))


def _rho_a(blk, agg, seed):
    n = len(blk.keys)
    root = RP.excess_halfagg_root(TAG, [RP.excess_halfagg_leaf(TAG, agg[33 * i:33 * i + 33], blk.keys[i], blk.msgs[i]) for i in range(n)])
    return RP.block_agg_weight(RP.block_seeds(seed)[1], n, root, agg[-32:])


# ----------------------------------------------------------------------------- 1. accept: one MSM, every key lifted once; the existing call is as it was
@pytest.mark.parametrize("nkeys", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_accept(gpu, handles, name, nkeys):
    nat = handles(name)
    blk, agg = _cut(handles, name, nkeys)
    assert nat.excess_halfagg(blk.keys, blk.msgs, blk.sigs) == agg and nat.excess_halfagg_verify(blk.keys, blk.msgs, agg) is True
    assert _both(nat, blk, agg) == (True, ([VALID] * NPROOFS, [OK] * nkeys, [OK] * 2), None)
    assert nat.verify_block_agg(*_args(blk, agg), bindings=blk.bindings) is True        # a fresh seed
    sh, nr = nat.shape, len(nat.st.rds)
    ninit = (2 if name == "bin_test" else 4) + nr
    terms = 1 + sh["lin_len"] + sh["norm_len"] + NPROOFS * (ninit + 2 * sh["rounds"]) + len(blk.en) + 2 * nkeys
    assert _counts(nat) == (1, terms, nkeys, ROWS * nr)
    assert nat.verify_block(*blk.args(), bindings=blk.bindings, seed=SEED, want_status=True, want_point=True) == (True, ([VALID] * NPROOFS, [OK] * nkeys, [OK] * 2), None)


# ----------------------------------------------------------------------------- 2. the formula, on a block that is wrong in all three parts
@pytest.mark.parametrize("nkeys", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_formula(gpu, oracle_lib, handles, name, nkeys):
    nat, ec = handles(name), oracle_lib
    blk, agg = _cut(handles, name, nkeys)
    _tamper_proof(blk, 1)
    blk.claims[0] = (blk.claims[0][0] + 1,) + tuple(blk.claims[0][1:])
    agg = _with_s(agg, (_s_agg(agg) + 3) % N)
    for seed in (SEED, SEED2):
        V, _, S = _parts(nat, gpu, blk, seed)
        kacc, kst, Kp = nat.excess_halfagg_verify(blk.keys, blk.msgs, agg, want_status=True, want_point=True)
        assert None not in (V, Kp, S) and (kacc, kst) == (False, [MISMATCH] * nkeys)
        acc, status, point = _both(nat, blk, agg, seed)
        assert not acc and point is not None and point == _sum3(ec, (V, ec.mul(_rho_a(blk, agg, seed), Kp), S))
        assert status[1] == kst and status[0][1] == INVALID and status[2][0] == MISMATCH
        assert status[0] == nat.verify_each(blk.coms[:NPROOFS], blk.proofs, bindings=blk.bindings)
        assert status[2] == nat.excess_sums_each(blk.coms, blk.ss, blk.en, blk.claims, blk.ks, blk.keys)


# ----------------------------------------------------------------------------- 3. each part alone rejects, with the stated statuses
@pytest.mark.parametrize("nkeys", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_each_part_alone_rejects(gpu, oracle_lib, handles, name, nkeys):
    nat, ec = handles(name), oracle_lib
    good = ([VALID] * NPROOFS, [OK] * nkeys, [OK] * 2)
    # the proofs
    blk, agg = _cut(handles, name, nkeys)
    _tamper_proof(blk, 3)
    acc, status, point = _both(nat, blk, agg)
    assert not acc and point is not None and status == ([INVALID if b == 3 else VALID for b in range(NPROOFS)], good[1], good[2])
    # the aggregate: its scalar, an R row, a message under it; s_agg that is no scalar
    blk, agg = _cut(handles, name, nkeys)
    last = nkeys - 1
    flipped = agg[:33 * last + 32] + bytes([agg[33 * last + 32] ^ 1]) + agg[33 * nkeys:]
    for bent in (_with_s(agg, (_s_agg(agg) + 1) % N), flipped):
        acc, status, point = _both(nat, blk, bent)
        assert not acc and point is not None and status == (good[0], [MISMATCH] * nkeys, good[2])
    acc, status, point = _both(nat, blk, _with_s(agg, N))
    assert not acc and status == (good[0], [NOT_CANONICAL] * nkeys, good[2])
    acc, status, _ = _both(nat, blk, agg[:33 * last + 32] + b"\x02" + agg[33 * nkeys:])
    assert not acc and status == (good[0], [MISMATCH] * last + [BAD_R], good[2])
    blk.msgs[last] = blk.msgs[last][::-1]
    acc, status, point = _both(nat, blk, agg)
    assert not acc and point is not None and status == (good[0], [MISMATCH] * nkeys, good[2])
    # a key that does not lift: BAD_KEY there and for its sum; the other keys get the equation's verdict over what is left
    blk, agg = _cut(handles, name, nkeys)
    blk.keys[0] = blk.keys[0][:32] + b"\x02"
    acc, status, _ = _both(nat, blk, agg)
    assert not acc and status == (good[0], [BAD_KEY] + [MISMATCH] * last, [BAD_KEY, OK])
    # the sums
    blk, agg = _cut(handles, name, nkeys)
    blk.claims[1] = (blk.claims[1][0] + 1,) + tuple(blk.claims[1][1:])
    acc, status, point = _both(nat, blk, agg)
    assert not acc and point is not None and status == (good[0], good[1], [OK, MISMATCH])


# ----------------------------------------------------------------------------- 4. arguments
def _raw(nat, blk, agg, with_sigs=False, key_offset=0):
    """the call on a capi.RpBlock filled by hand, so that sigs and key_offset can be what the wrapper never passes"""
    arrs, n = nat.block_arrays(*blk.args(), blk.bindings)
    rb = capi.RpBlock(key_offset=key_offset, **n)
    for field, a in arrs:
        if a is not None and (field != "sigs" or with_sigs):
            setattr(rb, field, a.ctypes.data)
    ag = np.frombuffer(agg, dtype=np.uint8)
    return nat.verify_block_call(rb, SEED, agg=ag.ctypes.data)


def test_arguments(gpu, handles):
    nat = handles("rec_test")
    blk, agg = _cut(handles, "rec_test", 3)
    assert _raw(nat, blk, agg) is True
    for kw in (dict(with_sigs=True), dict(key_offset=1), dict(with_sigs=True, key_offset=2**40)):
        with pytest.raises(capi.BpppError, match=r"rp_verify_block_agg: blk->sigs must be NULL and blk->key_offset 0"):
            _raw(nat, blk, agg, **kw)
    with pytest.raises(capi.BpppError, match=r"blk->key_offset 0"):
        nat.verify_block_agg_device(*_args(blk, agg), bindings=blk.bindings, offsets=(0, 5, 0))
    lib, acc = gpu.lib, C.c_int(7)
    rb = capi.RpBlock()                                                                  # nothing to check: accepted, the aggregate is not looked at
    assert lib.bppp_rp_verify_block_agg(nat.h, C.byref(rb), None, None, C.byref(acc), None, None) == 0 and acc.value == 1
    acc.value = 7
    assert lib.bppp_rp_verify_block_agg_device(nat.h, C.byref(rb), None, None, C.byref(acc), None, None) == 0 and acc.value == 1
    assert lib.bppp_rp_verify_block_agg(nat.h, None, None, None, C.byref(acc), None, None) == -1 and lib.bppp_rp_verify_block_agg(nat.h, C.byref(rb), None, None, None, None, None) == -1
    # keys without an aggregate
    arrs, n = nat.block_arrays(*blk.args(), blk.bindings)
    rb = capi.RpBlock(**n)
    for field, a in arrs:
        if a is not None and field != "sigs":
            setattr(rb, field, a.ctypes.data)
    sd = np.frombuffer(SEED, dtype=np.uint8)
    assert lib.bppp_rp_verify_block_agg(nat.h, C.byref(rb), None, C.c_void_p(sd.ctypes.data), C.byref(acc), None, None) == -1 and b"rp_verify_block: null input" in lib.bppp_last_error(gpu.h)
    # the one-pass limit and its text are the block call's
    tl = capi.load_test_library()
    assert tl.bppp_test_rp_set_flat_chunk(nat.h, 8) == 0                                 # two keys a pass
    try:
        with pytest.raises(capi.BpppError, match=r"rp_verify_block: the block does not fit one pass: nkeys = 3 against the key pass of 2"):
            nat.verify_block_agg(*_args(blk, agg), bindings=blk.bindings)
    finally:
        assert tl.bppp_test_rp_set_flat_chunk(nat.h, 0) == 0
    assert nat.verify_block_agg(*_args(blk, agg), bindings=blk.bindings) is True


# ----------------------------------------------------------------------------- 5. nothing rests on what an earlier call left in the workspaces
@pytest.mark.parametrize("name", NAMES)
def test_after_poisoned_workspaces(gpu, oracle_lib, handles, name):
    """the block of three keys warms the buffers, poison, then the block of one key: accepted, and with s_agg + 1, whose point is rho_A B by the oracle"""
    nat, tl, n = handles(name), capi.load_test_library(), C.c_uint64(0)
    warm, wagg = _cut(handles, name, 3)
    blk, agg = _cut(handles, name, 1)
    bent = _with_s(agg, (_s_agg(agg) + 1) % N)
    rho_b = oracle_lib.mul(_rho_a(blk, bent, SEED), RP._excess_bases(nat.st)[2])
    want = [(True, ([VALID] * NPROOFS, [OK], [OK] * 2), None), (False, ([VALID] * NPROOFS, [MISMATCH], [OK] * 2), rho_b)]
    for byte in (0x00, 0xA5):
        for a, expect in zip((agg, bent), want):
            assert nat.verify_block_agg(*_args(warm, wagg), bindings=warm.bindings) is True
            assert tl.bppp_test_ctx_poison(gpu.h, byte, C.byref(n)) == 0 and n.value > 0
            assert tl.bppp_test_rp_poison(nat.h, byte, C.byref(n)) == 0 and n.value > 0
            assert _both(nat, blk, a) == expect, byte
