"""Per-proof public amounts (bppp_rp_*_pub): one handle serves proofs whose fees (typed reciprocal `public` amounts) or net public amounts
(conserved RangeProof.Binary) differ from proof to proof.  Proof b under a *_pub call must behave exactly as proof b under a handle created
with proof b's amounts: the prover's files byte for byte (every prover route), the verifier's statuses, challenges, per-proof points E_b
and, with the weights of bppp_rp_verify_shard_device at the same job positions, the combined point."""
import ctypes as C
import hashlib
import json
import os
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import encoding as E
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import BpppError, array_to_point, scalars_to_array
from test_rangeproof import EXAMPLES

pytestmark = pytest.mark.gpu

SEED = hashlib.sha256(b"public amounts seed").digest()
VALID, INVALID = 0, 1
ERR_ARG = -1
PTS = O.hash_points(b"public amounts", 120)
FEE_TYPE = 7


# ----------------------------------------------------------------------------- a small typed conserved shape: 2 inputs + 2 outputs of 32 bits, one public fee
def _typed_setup(gpu, fee):
    rds = [RP.make_range_data(4, 0, 2**32, False, False, False), RP.make_range_data(4, 0, 2**32, False, False, False),
           RP.make_range_data(4, 0, 2**32, False, True, False), RP.make_range_data(4, 0, 2**32, False, True, False)]
    return RP.setup(RP.GpuBackend(gpu), PTS, True, [(True, FEE_TYPE, fee)], rds, "NL")       # the fee is a public OUTPUT: in1 + in2 = out1 + out2 + fee


def _typed_inputs(fees, seed):
    rnd = random.Random(seed)
    out = []
    for fee in fees:
        total = fee + rnd.randrange(2**31)
        i1 = rnd.randrange(max(total - (2**32 - 1), 0), min(total, 2**32 - 1) + 1)
        o1 = rnd.randrange(total - fee + 1)
        out.append([(i1, FEE_TYPE, rnd.randrange(O.N)), (total - i1, FEE_TYPE, rnd.randrange(O.N)), (o1, FEE_TYPE, rnd.randrange(O.N)),
                    (total - fee - o1, FEE_TYPE, rnd.randrange(O.N))])
    return out


class _Handles:
    """the handle under test (created with fee 0) and one reference handle per distinct fee, created with that fee"""

    def __init__(self, gpu, make):
        self.gpu, self.make, self.refs = gpu, make, {}
        self.main = make(0)

    def ref(self, fee):
        if fee not in self.refs:
            self.refs[fee] = self.make(fee)
        return self.refs[fee]

    def close(self):
        for h in [self.main] + list(self.refs.values()):
            h.close()


@pytest.fixture(scope="module")
def typed(gpu):
    hs = _Handles(gpu, lambda fee: RP.NativeRangeProofs(gpu, _typed_setup(gpu, fee)))
    yield hs
    hs.close()


def _binary_schema(net):
    schema = json.load(open(os.path.join(EXAMPLES, "bin_test", "schema.json")))
    return dict(schema, public=[{"amount": net, "isOutput": False}])


@pytest.fixture(scope="module")
def binary(gpu):
    hs = _Handles(gpu, lambda net: BRP.NativeBinaryRangeProofs(gpu, BRP.setup_from_schema(RP.GpuBackend(gpu), _binary_schema(net))))
    yield hs
    hs.close()


def _binary_inputs(nets, seed):
    """bin_test's shape: one output in [3, 2^64), two assumed inputs; net + in1 + in2 - out = 0"""
    rnd = random.Random(seed)
    out = []
    for net in nets:
        i1, i2 = rnd.randrange(100, 1000), rnd.randrange(100, 1000)
        out.append([(net + i1 + i2, rnd.randrange(O.N)), (i1, rnd.randrange(O.N)), (i2, rnd.randrange(O.N))])
    return out


def _ref_files(hs, amounts, inputs, prefixes):
    """each proof made on the handle created with its own amounts (one call per distinct amount)"""
    out = [None] * len(inputs)
    for a in sorted(set(amounts)):
        idx = [b for b in range(len(inputs)) if amounts[b] == a]
        got = hs.ref(a).prove_batch([inputs[b] for b in idx], [prefixes[b] for b in idx])
        for b, f in zip(idx, got):
            out[b] = f
    return out


class _options:
    def __init__(self, nat, **kw):
        self.nat, self.kw = nat, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.nat.set_option(k, v)

    def __exit__(self, *exc):
        defaults = {"comb_min": 1024, "comb_bits": 0, "split_min": 4096, "fold_points": 0, "host_algebra": 0, "culprits": 0, "host_oracle_max": 2**64 - 1}
        for k in self.kw:
            self.nat.set_option(k, defaults[k])


def _up(gpu, bs):
    raw = b"".join(bs)
    return gpu.to_device(np.frombuffer(raw + b"\0" * (-len(raw) % 8), dtype=np.uint64))


def _shard_point(nat, files, offset, public_amounts=None):
    """bppp_rp_verify_shard{,_pub}_device: (accept, combined point as 8 words)"""
    gpu = nat.gpu
    dc, dp = _up(gpu, [c for c, _ in files]), _up(gpu, [p for _, p in files])
    try:
        acc, out = C.c_int(0), np.zeros(8, dtype=np.uint64)
        sd = np.frombuffer(SEED, dtype=np.uint8)
        args = (C.c_void_p(sd.ctypes.data), C.byref(acc), None, None, C.c_void_p(out.ctypes.data))
        if public_amounts is None:
            rc = gpu.lib.bppp_rp_verify_shard_device(nat.h, len(files), offset, C.c_void_p(dc), C.c_void_p(dp), *args)
        else:
            pa = nat._public_words(public_amounts, len(files))
            dpa = gpu.to_device(pa)
            try:
                rc = gpu.lib.bppp_rp_verify_shard_pub_device(nat.h, len(files), offset, C.c_void_p(dc), C.c_void_p(dp), C.c_void_p(dpa), *args)
            finally:
                gpu.free(dpa)
        gpu._check(rc, "bppp_rp_verify_shard_device")
        return bool(acc.value), out
    finally:
        gpu.free(dc); gpu.free(dp)


def _sum(gpu, pts):
    return gpu.sum_points(np.stack(pts))


# ----------------------------------------------------------------------------- 1. typed prover bytes on every route
def test_typed_prover_bytes_every_route(typed, gpu):
    fees = [0, 5, 5, 2**32 + 7, 17, 0, 1234567]                  # zero, a repeated one, one above any single range
    inputs = _typed_inputs(fees, 1)
    prefixes = [b"pub typed %02d" % b for b in range(len(fees))]
    want = _ref_files(typed, fees, inputs, prefixes)
    pubs = [[f] for f in fees]
    nat = typed.main
    assert nat.public_count() == 1
    got = nat.prove_batch(inputs, prefixes, public_amounts=pubs)       # device phases, point-folding argument
    assert got == want
    for b in (0, 3, 6):                                                    # the host protocol with a setup of that fee
        st = _typed_setup(gpu, fees[b])
        proof = RP.prove(st, RP.witness(st, inputs[b]), RP.sha256_oracle(), RP.hash_to_scalar(prefixes[b]))
        assert got[b] == E.encode_proof(4, proof), b
    with _options(nat, host_algebra=1):
        assert nat.prove_batch(inputs, prefixes, public_amounts=pubs) == want
    with _options(nat, split_min=2):                                       # two half-batches: the twin gets its slice of the amounts
        assert nat.prove_batch(inputs, prefixes, public_amounts=pubs) == want
    with _options(nat, comb_min=1, comb_bits=7):                           # comb table, one stream of kernels, host oracle
        assert nat.prove_batch(inputs, prefixes, public_amounts=pubs) == want
        with _options(nat, host_oracle_max=0):
            assert nat.prove_batch(inputs, prefixes, public_amounts=pubs) == want
        with _options(nat, fold_points=1):
            assert nat.prove_batch(inputs, prefixes, public_amounts=pubs) == want
        with _options(nat, split_min=2):
            assert nat.prove_batch(inputs, prefixes, public_amounts=pubs) == want


# ----------------------------------------------------------------------------- 2. typed verify: accept, challenges, combined point
@pytest.mark.parametrize("B", [6, 64])
def test_typed_verify_matches_per_fee_handles(typed, gpu, B):
    rnd = random.Random(B)
    fees = [rnd.choice([0, 1, 99, 2**20, 2**32 + 3]) for _ in range(B)]
    fees[0] = 99
    inputs = _typed_inputs(fees, B)
    prefixes = [b"pub verify %04d" % b for b in range(B)]
    nat = typed.main
    files = nat.prove_batch(inputs, prefixes, public_amounts=[[f] for f in fees])
    coms, prfs = [c for c, _ in files], [p for _, p in files]
    ok, status, chs = nat.verify_batch(coms, prfs, SEED, want_status=True, want_challenges=True, public_amounts=[[f] for f in fees])
    assert ok and status == [VALID] * B
    assert not nat.verify_batch(coms, prfs, SEED)                          # the handle's own fee (0) does not open them
    for b in range(B):
        _, _, ref_ch = typed.ref(fees[b]).verify_batch([coms[b]], [prfs[b]], SEED, want_challenges=True)
        assert chs[b] == ref_ch[0], b
    acc, got = _shard_point(nat, files, 11, public_amounts=[[f] for f in fees])
    assert acc and array_to_point(got) is None
    # the combined point of a batch that does NOT verify, against the sum of single-proof shard points at the same job positions
    bad = [[f + (1 if b % 5 == 2 else 0)] for b, f in enumerate(fees)]
    acc, got = _shard_point(nat, files, 11, public_amounts=bad)
    parts = [_shard_point(typed.ref(bad[b][0]), [files[b]], 11 + b)[1] for b in range(B)]
    assert not acc and array_to_point(got) == _sum(gpu, parts) and array_to_point(got) is not None


def test_typed_verify_split_route_above_1024(typed, gpu):
    """1100 proofs: the public scalars take the split route (k_trrp_pre -> k_trrp_pos -> k_trrp_lin) with per-proof amounts; blocks of
    100 proofs share a fee, and each block's shard point on its fee's handle (the one-kernel route, 100 proofs) must add up to the whole"""
    B, blk = 1100, 100
    fees = [(b // blk) * 1000003 for b in range(B)]
    inputs = _typed_inputs(fees, 5)
    prefixes = [b"pub split %05d" % b for b in range(B)]
    nat = typed.main
    pubs = [[f] for f in fees]
    files = nat.prove_batch(inputs, prefixes, public_amounts=pubs)
    coms, prfs = [c for c, _ in files], [p for _, p in files]
    assert nat.verify_batch(coms, prfs, SEED, public_amounts=pubs)
    wrong = [list(p_) for p_ in pubs]
    wrong[1050][0] += 1
    acc, got = _shard_point(nat, files, 0, public_amounts=wrong)
    assert not acc
    parts, s = [], 0
    while s < B:                                                           # runs of one fee, each on its fee's handle at its job positions
        e = s
        while e < B and wrong[e] == wrong[s]:
            e += 1
        parts.append(_shard_point(typed.ref(wrong[s][0]), files[s:e], s)[1])
        s = e
    assert len(parts) == 13 and array_to_point(got) == _sum(gpu, parts)
    dc, dp = _up(gpu, coms), _up(gpu, prfs)
    try:
        st = nat.verify_each_device(B, dc, dp, public_amounts=wrong)
    finally:
        gpu.free(dc); gpu.free(dp)
    assert [b for b, s_ in enumerate(st) if s_] == [1050]


# ----------------------------------------------------------------------------- 3. wrong amounts are pinned to their proofs
@pytest.mark.parametrize("culprits", [0, 1])
def test_wrong_amounts_identify_exactly_those_proofs(typed, culprits):
    fees = [10, 20, 30, 40, 50, 60, 70, 80, 90]
    inputs = _typed_inputs(fees, 3)
    nat = typed.main
    files = nat.prove_batch(inputs, [b"wrong %d" % b for b in range(len(fees))], public_amounts=[[f] for f in fees])
    coms, prfs = [c for c, _ in files], [p for _, p in files]
    wrong = list(fees)
    wrong[1], wrong[6] = wrong[6], wrong[1]
    wrong[4] += 1
    with _options(nat, culprits=culprits):
        ok, status, _ = nat.verify_batch(coms, prfs, SEED, want_status=True, public_amounts=[[f] for f in wrong])
        assert not ok and [b for b, s_ in enumerate(status) if s_] == [1, 4, 6] and all(status[b] == INVALID for b in (1, 4, 6))
        ok, status, _ = nat.verify_batch(coms, prfs, SEED, want_status=True, public_amounts=[[f] for f in fees])
        assert ok and status == [VALID] * len(fees)


# ----------------------------------------------------------------------------- 4. the per-proof pass
def test_verify_each_matches_per_fee_handles(typed, gpu):
    fees = [3, 3, 0, 2**32 + 2**30, 77, 5]
    inputs = _typed_inputs(fees, 4)
    nat = typed.main
    files = nat.prove_batch(inputs, [b"each %d" % b for b in range(len(fees))], public_amounts=[[f] for f in fees])
    coms, prfs = [c for c, _ in files], [p for _, p in files]
    for claimed in (fees, [f + (b == 2) for b, f in enumerate(fees)]):
        st, pts = nat.verify_each(coms, prfs, want_points=True, public_amounts=[[f] for f in claimed])
        for b in range(len(fees)):
            rs, rp_ = typed.ref(claimed[b]).verify_each([coms[b]], [prfs[b]], want_points=True)
            assert (st[b], pts[b]) == (rs[0], rp_[0]), b
        dc, dp = _up(gpu, coms), _up(gpu, prfs)
        try:
            assert nat.verify_each_device(len(fees), dc, dp, want_points=True, public_amounts=[[f] for f in claimed]) == (st, pts)
        finally:
            gpu.free(dc); gpu.free(dp)
    assert st == [VALID, VALID, INVALID, VALID, VALID, VALID]


# ----------------------------------------------------------------------------- 5. conserved RangeProof.Binary, per-proof net_public
def test_binary_per_proof_net_public(binary, gpu):
    nets = [2, 2, -22, 0, 2**40, 7, -1]                                    # negative nets in two's complement, as bppp_rp_create_binary takes them
    inputs = _binary_inputs(nets, 9)
    prefixes = [b"pub binary %02d" % b for b in range(len(nets))]
    want = _ref_files(binary, nets, inputs, prefixes)
    nat = binary.main
    assert nat.public_count() == 1
    got = nat.prove_batch(inputs, prefixes, public_amounts=nets)            # host-algebra route (small batch, no table)
    assert got == want
    for b in (2, 4):
        st = BRP.setup_from_schema(RP.GpuBackend(gpu), _binary_schema(nets[b]))
        assert got[b] == E.encode_proof(2, BRP.prove(st, BRP.witness(st, inputs[b]), RP.sha256_oracle(), RP.hash_to_scalar(prefixes[b]))), b
    with _options(nat, comb_min=1, comb_bits=7):                            # the device binary prover over a comb table
        assert nat.prove_batch(inputs, prefixes, public_amounts=nets) == want
        with _options(nat, host_oracle_max=0):
            assert nat.prove_batch(inputs, prefixes, public_amounts=nets) == want
    coms, prfs = [c for c, _ in got], [p for _, p in got]
    ok, status, chs = nat.verify_batch(coms, prfs, SEED, want_status=True, want_challenges=True, public_amounts=nets)
    assert ok and status == [VALID] * len(nets)
    for b in range(len(nets)):
        assert chs[b] == binary.ref(nets[b]).verify_batch([coms[b]], [prfs[b]], SEED, want_challenges=True)[2][0]
    wrong = list(nets)
    wrong[0], wrong[2] = wrong[2], wrong[0]
    wrong[5] += 1
    for culprits in (0, 1):
        with _options(nat, culprits=culprits):
            ok, status, _ = nat.verify_batch(coms, prfs, SEED, want_status=True, public_amounts=wrong)
            assert not ok and [b for b, s_ in enumerate(status) if s_] == [0, 2, 5]
    acc, got_pt = _shard_point(nat, got, 3, public_amounts=wrong)
    parts = [_shard_point(binary.ref(wrong[b]), [got[b]], 3 + b)[1] for b in range(len(nets))]
    assert not acc and array_to_point(got_pt) == _sum(gpu, parts)
    st, pts = nat.verify_each(coms, prfs, want_points=True, public_amounts=wrong)
    for b in range(len(nets)):
        rs, rp_ = binary.ref(wrong[b]).verify_each([coms[b]], [prfs[b]], want_points=True)
        assert (st[b], pts[b]) == (rs[0], rp_[0]), b
    # a proof whose amounts do not balance with its own net_public is refused, named by its index
    off = list(nets)
    off[3] = 1
    with pytest.raises(BpppError, match="proof 3"):
        nat.prove_batch(inputs, prefixes, public_amounts=off)


# ----------------------------------------------------------------------------- 6. scale: config 4 (128 x 64-bit typed, conserved), a public input per proof
def test_config4_scale_with_a_public_input_per_proof(gpu):
    schema = json.load(open(os.path.join(EXAMPLES, "128by64", "schema.json")))
    schema = dict(schema, typed=True, public=[{"amount": 128 * 10000, "type": 0}])
    st = RP.setup_from_schema(RP.GpuBackend(gpu), schema)
    nat = RP.NativeRangeProofs(gpu, st)
    assert nat.public_count() == 1
    B = 256
    rng = np.random.default_rng(6)
    inputs, pubs = [], []
    for b in range(B):
        vals = [int(x) for x in rng.integers(1000, 20000, size=128)]
        inputs.append([(v, 0, int(bl)) for v, bl in zip(vals, rng.integers(1, 2**63, size=128, dtype=np.uint64))])
        pubs.append([sum(vals)])                                             # the public input each proof's outputs add up to
    files = nat.prove_batch(inputs, [b"cfg4 pub %04d" % b for b in range(B)], public_amounts=pubs)
    coms, prfs = [c for c, _ in files], [p for _, p in files]
    assert nat.verify_batch(coms, prfs, SEED, public_amounts=pubs)
    st3 = RP.setup_from_schema(RP.GpuBackend(gpu), dict(schema, public=[{"amount": pubs[3][0], "type": 0}]))
    proof = E.decode_proof(4, st3.rounds, st3.final_lens, E.decode_commitments(128, coms[3], E.gpu_lift_x(gpu))[0], prfs[3], E.gpu_lift_x(gpu))
    assert RP.verify(st3, proof, RP.sha256_oracle())
    bad = list(prfs)
    pf = bytearray(bad[137]); pf[5] ^= 1; bad[137] = bytes(pf)
    ok, status, _ = nat.verify_batch(coms, bad, SEED, want_status=True, public_amounts=pubs)
    assert not ok and [b for b, s_ in enumerate(status) if s_] == [137]
    nat.close()


# ----------------------------------------------------------------------------- 7. NULL equivalence, argument errors, public_count
def test_null_amounts_and_argument_errors(typed, gpu):
    nat = typed.main
    fees = [0, 0, 0, 0]
    inputs = _typed_inputs(fees, 8)
    prefixes = [b"null %d" % b for b in range(4)]
    files = nat.prove_batch(inputs, prefixes)
    lib = gpu.lib
    cb = np.frombuffer(b"".join(c for c, _ in files), dtype=np.uint8)
    pb = np.frombuffer(b"".join(p for _, p in files), dtype=np.uint8)
    sd = np.frombuffer(SEED, dtype=np.uint8)
    vp = lambda a: C.c_void_p(a.ctypes.data)

    def run(fn, *pub):
        acc, st_, xy = C.c_int(7), np.zeros(4, dtype=np.uint32), np.zeros(8, dtype=np.uint64)
        rc = fn(nat.h, 4, vp(cb), vp(pb), *pub, vp(sd), C.byref(acc), vp(st_), None, vp(xy))
        return rc, acc.value, list(st_), list(xy)
    corrupt = bytearray(pb); corrupt[nat.shape["proof_bytes"] + 3] ^= 1
    for pbuf in (pb, np.frombuffer(bytes(corrupt), dtype=np.uint8)):
        pb = pbuf
        assert run(lib.bppp_rp_verify_batch_pub, None) == run(lib.bppp_rp_verify_batch)
    st0 = np.zeros(4, dtype=np.uint32)
    st1 = np.zeros(4, dtype=np.uint32)
    assert lib.bppp_rp_verify_each_pub(nat.h, 4, vp(cb), vp(pb), None, vp(st0), None) == 0
    assert lib.bppp_rp_verify_each(nat.h, 4, vp(cb), vp(pb), vp(st1), None) == 0
    assert list(st0) == list(st1) == [VALID, INVALID, VALID, VALID]
    # a proof that does not balance with its own fee is refused, named by its index in the whole batch
    with pytest.raises(BpppError, match="proof 2"):
        nat.prove_batch(inputs, prefixes, public_amounts=[[0], [0], [1], [0]])
    with _options(nat, split_min=2), pytest.raises(BpppError, match="proof 3"):
        nat.prove_batch(inputs, prefixes, public_amounts=[[0], [0], [0], [5]])
    # a non-canonical typed amount (the Python wrapper reduces mod N; the C entry points check)
    bad = scalars_to_array([0, 0, O.N, 0])
    acc = C.c_int(0)
    assert lib.bppp_rp_verify_batch_pub(nat.h, 4, vp(cb), vp(pb), vp(bad), vp(sd), C.byref(acc), None, None, None) == ERR_ARG
    cf, pf = np.zeros(4 * nat.shape["coms_bytes"], dtype=np.uint8), np.zeros(4 * nat.shape["proof_bytes"], dtype=np.uint8)
    amt = scalars_to_array([v % 2**256 for row in inputs for v, _, _ in row])
    typ = scalars_to_array([t for row in inputs for _, t, _ in row])
    bld = scalars_to_array([x for row in inputs for _, _, x in row])
    pre = np.frombuffer(b"".join(prefixes), dtype=np.uint8)
    assert lib.bppp_rp_prove_batch_pub(nat.h, 4, vp(amt), vp(typ), vp(bld), vp(bad), vp(pre), len(prefixes[0]), vp(cf), vp(pf)) == ERR_ARG
    # handles without public amounts: untyped, and binary without conservation
    rds = [RP.make_range_data(4, 0, 2**32, False, False, False)]
    untyped = RP.NativeRangeProofs(gpu, RP.setup(RP.GpuBackend(gpu), PTS, False, [(True, FEE_TYPE, 5)], rds, "NL"))
    nb = BRP.NativeBinaryRangeProofs(gpu, BRP.setup_from_schema(RP.GpuBackend(gpu), dict(_binary_schema(2), conserved=False)))
    try:
        assert untyped.public_count() == 0 and nb.public_count() == 0
        one = scalars_to_array([0])
        for h in (untyped, nb):
            st_ = np.zeros(1, dtype=np.uint32)
            assert lib.bppp_rp_verify_each_pub(h.h, 1, vp(cb), vp(pb), vp(one), vp(st_), None) == ERR_ARG
            assert lib.bppp_rp_verify_batch_pub(h.h, 1, vp(cb), vp(pb), vp(one), vp(sd), C.byref(acc), None, None, None) == ERR_ARG
            xy = np.full(8, 7, dtype=np.uint64)
            assert lib.bppp_rp_verify_batch_pub(h.h, 0, None, None, vp(one), vp(sd), C.byref(acc), None, None, vp(xy)) == 0 and acc.value == 1
            assert not xy.any()                     # an empty batch zeroes combined_xy, from host files as from HBM
    finally:
        untyped.close(); nb.close()
    n = C.c_size_t(9)
    assert lib.bppp_rp_public_count(None, C.byref(n)) == ERR_ARG
    assert typed.ref(5).public_count() == 1
