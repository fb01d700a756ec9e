"""bppp_rp_verify_mixed*: range proofs of SEVERAL setups (every example the reference ships: typed-reciprocal and binary, norm-linear and
inner-product argument) verified in one call with one combined MSM.  The job is the groups concatenated in order, so the combined point is
exactly the sum of every group's bppp_rp_verify_shard_device point at its job offset with the same seed; statuses come back in job order;
setups derived from one point stream share their basis terms (the merge), setups of another stream get their own."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from bulletproofspp_amd import encoding as E
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import BpppError, array_to_point, load_test_library, points_to_array
from test_rangeproof import EXAMPLES

pytestmark = pytest.mark.gpu

ALL = ["32bit", "64bit", "rec_test", "32by64", "64by64", "96by64", "128by64", "bin_test"]
B = 3
SEED = hashlib.sha256(b"mixed job seed").digest()
P = 2**256 - 2**32 - 977


def _handle(gpu, name, basis_seed=None):
    schema = json.load(open(os.path.join(EXAMPLES, name, "schema.json")))
    if basis_seed is not None:
        schema["basisSeed"] = basis_seed
    binary = bool(schema.get("binary", False))
    if binary:
        nat = BRP.NativeBinaryRangeProofs(gpu, BRP.setup_from_schema(RP.GpuBackend(gpu), schema))
    else:
        nat = RP.NativeRangeProofs(gpu, RP.setup_from_schema(RP.GpuBackend(gpu), schema))
    wit_json = json.load(open(os.path.join(EXAMPLES, name, "witness.json")))
    inputs = []
    for j in range(B):
        rows = RP.inputs_from_witness(wit_json, b"mixed %s %d" % (name.encode(), j))
        inputs.append([(v, bl) for v, _, bl in rows] if binary else rows)
    files = nat.prove_batch(inputs, [b"mixed random seed %d" % j for j in range(B)])
    return nat, [c for c, _ in files], [p for _, p in files]


@pytest.fixture(scope="module")
def examples(gpu):
    hs = {name: _handle(gpu, name) for name in ALL}
    yield hs
    for nat, _, _ in hs.values():
        nat.close()


def _up(gpu, bs):
    raw = b"".join(bs) or b"\0"
    return gpu.to_device(np.frombuffer(raw + b"\0" * (-len(raw) % 8), dtype=np.uint8).view(np.uint64))


def _mixed_device(gpu, groups, index_offset=0, seed=SEED):
    bufs = [(_up(gpu, cf), _up(gpu, pf)) for _, cf, pf in groups]
    try:
        return RP.verify_mixed_device(gpu, [(nat, len(pf), dc, dp) for (nat, _, pf), (dc, dp) in zip(groups, bufs)], seed, index_offset)
    finally:
        for dc, dp in bufs:
            gpu.free(dc); gpu.free(dp)


def _shard(gpu, nat, cf, pf, offset, seed=SEED):
    """bppp_rp_verify_shard_device with status: (accept, status, point)"""
    dc, dp = _up(gpu, cf), _up(gpu, pf)
    try:
        acc, out = C.c_int(0), np.zeros(8, dtype=np.uint64)
        st = np.zeros(max(len(pf), 1), dtype=np.uint32)
        sd = np.frombuffer(seed, dtype=np.uint8)
        rc = gpu.lib.bppp_rp_verify_shard_device(nat.h, len(pf), offset, C.c_void_p(dc), C.c_void_p(dp), C.c_void_p(sd.ctypes.data), C.byref(acc),
                                                 C.c_void_p(st.ctypes.data), None, C.c_void_p(out.ctypes.data))
        gpu._check(rc, "bppp_rp_verify_shard_device")
        return bool(acc.value), [int(v) for v in st[:len(pf)]], array_to_point(out)
    finally:
        gpu.free(dc); gpu.free(dp)


def _sum_of_shards(gpu, groups, index_offset=0):
    pts, start = [], index_offset
    for nat, cf, pf in groups:
        if pf:
            pts.append(_shard(gpu, nat, cf, pf, start)[2])
        start += len(pf)
    return gpu.sum_points(points_to_array(pts)) if pts else None


def _terms(gpu):
    t = C.c_uint64(0)
    assert load_test_library().bppp_test_last_mixed_msm_terms(gpu.h, C.byref(t)) == 0
    return t.value


def _per_proof(nat):
    s = nat.shape
    return (2 if isinstance(nat, BRP.NativeBinaryRangeProofs) else 4) + s["nranges"] + 2 * s["rounds"]


def _basis_len(nat):
    return 1 + nat.shape["lin_len"] + nat.shape["norm_len"]


def _non_liftable_x():
    x = 5
    while pow((x ** 3 + 7) % P, (P - 1) // 2, P) == 1:
        x += 1
    return x


def _bad_job(examples):
    """group 2: a flipped bit in its second proof; group 5: its third proof's first commitment with an x that has no curve point"""
    groups = [list(examples[n]) for n in ALL]
    pf = bytearray(groups[2][2][1]); pf[5] ^= 2
    groups[2][2] = groups[2][2][:1] + [bytes(pf)] + groups[2][2][2:]
    nat5 = groups[5][0]
    cf = bytearray(groups[5][1][2]); sb = (nat5.shape["nranges"] + 7) // 8
    cf[sb:sb + 32] = E.put_field(_non_liftable_x())
    groups[5][1] = groups[5][1][:2] + [bytes(cf)]
    return [tuple(g) for g in groups]


def test_all_examples_in_one_call(gpu, examples):
    groups = [examples[n] for n in ALL]
    ok, status, pt = _mixed_device(gpu, groups)
    assert ok and status == [0] * (B * len(ALL))
    assert pt is None and _sum_of_shards(gpu, groups) is None
    assert RP.verify_mixed(gpu, groups, SEED, want_status=True) == (True, [0] * (B * len(ALL)))
    # one stream ("test points"): one family, whose union basis is the longest setup's
    assert _terms(gpu) == max(_basis_len(n) for n, _, _ in groups) + sum(B * _per_proof(n) for n, _, _ in groups)


def test_bad_proofs_are_found_in_job_order(gpu, examples):
    groups = _bad_job(examples)
    ok, status, pt = _mixed_device(gpu, groups)
    want = [0] * (B * len(ALL))
    want[2 * B + 1], want[5 * B + 2] = 1, 2
    assert not ok and status == want
    assert RP.verify_mixed(gpu, groups, SEED, want_status=True) == (False, want)


def test_combined_point_of_a_rejected_job_is_the_sum_of_the_shards(gpu, examples):
    groups = _bad_job(examples)
    ok, _, pt = _mixed_device(gpu, groups, index_offset=7)
    assert not ok and pt is not None
    assert pt == _sum_of_shards(gpu, groups, index_offset=7)


def test_second_basis_family(gpu, examples):
    other = _handle(gpu, "32by64", basis_seed="other points")
    try:
        bad = list(examples["64by64"])
        pf = bytearray(bad[2][0]); pf[40] ^= 1
        bad[2] = [bytes(pf)] + bad[2][1:]
        groups = [examples["32by64"], other, examples["64bit"], tuple(bad), examples["bin_test"]]
        ok, status, pt = _mixed_device(gpu, groups, index_offset=3)
        assert not ok and status == [0] * 9 + [1] + [0] * 5
        assert pt is not None and pt == _sum_of_shards(gpu, groups, index_offset=3)
        fam_a = [examples["32by64"][0], examples["64bit"][0], bad[0], examples["bin_test"][0]]
        assert _terms(gpu) == max(_basis_len(n) for n in fam_a) + _basis_len(other[0]) + sum(B * _per_proof(n) for n, _, _ in groups)
        ok, status, pt = _mixed_device(gpu, [examples["32by64"], other])
        assert ok and status == [0] * 6 and pt is None
    finally:
        other[0].close()


def test_the_merge_happens(gpu, examples):
    groups = [examples[n] for n in ("32by64", "64by64", "128by64")]
    ok, status, pt = _mixed_device(gpu, groups)
    assert ok and status == [0] * 9 and pt is None
    per = sum(B * _per_proof(n) for n, _, _ in groups)
    big = examples["128by64"][0]
    assert _terms(gpu) == 1 + big.shape["lin_len"] + big.shape["norm_len"] + per
    assert _terms(gpu) < sum(_basis_len(n) for n, _, _ in groups) + per


def test_one_group_equals_the_single_handle_call(gpu, examples):
    nat, cf, pf = _bad_job(examples)[2]                       # rec_test with its second proof corrupted
    want = _shard(gpu, nat, cf, pf, 11)
    assert not want[0] and want[1] == [0, 1, 0] and want[2] is not None
    assert _mixed_device(gpu, [(nat, cf, pf)], index_offset=11) == want
    a = _mixed_device(gpu, [(nat, cf[:2], pf[:2])], index_offset=11)
    b_ = _mixed_device(gpu, [(nat, cf[2:], pf[2:])], index_offset=13)
    assert a[1] + b_[1] == want[1]
    assert gpu.sum_points(points_to_array([a[2], b_[2]])) == want[2]
    good = examples["96by64"]
    assert _mixed_device(gpu, [good], index_offset=4) == _shard(gpu, *good, 4) == (True, [0, 0, 0], None)


def test_edge_cases(gpu, examples):
    n32, c32, p32 = examples["32by64"]
    nbin, cbin, pbin = examples["bin_test"]
    # empty groups beside non-empty ones take no part (not even the longer basis of 128by64)
    groups = [(examples["128by64"][0], [], []), examples["32by64"], (examples["64bit"][0], [], []), examples["bin_test"]]
    ok, status, pt = _mixed_device(gpu, groups, index_offset=2)
    assert ok and status == [0] * 6 and pt is None
    assert _terms(gpu) == max(_basis_len(n32), _basis_len(nbin)) + B * (_per_proof(n32) + _per_proof(nbin))
    # all groups empty, or no group at all: accepted
    assert _mixed_device(gpu, [(n32, [], []), (nbin, [], [])]) == (True, [], None)
    assert _mixed_device(gpu, []) == (True, [], None)
    assert RP.verify_mixed(gpu, [], SEED) is True
    assert RP.verify_mixed(gpu, [(n32, [], [])], SEED, want_status=True) == (True, [])
    # the same handle in two groups
    with pytest.raises(BpppError, match="two groups"):
        _mixed_device(gpu, [examples["32by64"], (n32, c32[:1], p32[:1])])
    with pytest.raises(BpppError, match="two groups"):
        RP.verify_mixed(gpu, [examples["32by64"], (n32, [], [])], SEED)
    # handles on two contexts
    import bulletproofspp_amd as b
    gpu2 = b.Bppp(0)
    try:
        schema = json.load(open(os.path.join(EXAMPLES, "32bit", "schema.json")))
        nat2 = RP.NativeRangeProofs(gpu2, RP.setup_from_schema(RP.GpuBackend(gpu2), schema))
        with pytest.raises(BpppError, match="different contexts"):
            RP.verify_mixed(gpu, [examples["32by64"], (nat2, examples["32bit"][1], examples["32bit"][2])], SEED)
        nat2.close()
    finally:
        gpu2.close()
    # wrong-length files: MALFORMED in the wrapper, no library call
    assert RP.verify_mixed(gpu, [examples["32by64"], (nbin, cbin, pbin[:2] + [pbin[2][:-1]])], SEED, want_status=True) == (False, [2] * 6)
    # the context still verifies after the refusals
    assert RP.verify_mixed(gpu, [examples["32by64"], examples["bin_test"]], SEED) is True
