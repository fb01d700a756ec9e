"""Per-proof transcript bindings (bppp_rp_*_bound*): proof b of a bound call must behave in every respect as a proof under a handle whose oracle
tag is oracle_tag + binding_b — every oracle message is  tag <> binding_b[32] <> show n <> show (length ps) <> text.

The reference for bytes and challenges is the HOST PROTOCOL code (rangeproof.prove / rangeproof_binary.prove and their verifier_challenges with
sha256_oracle(tag + binding), curve operations by the CPU oracle of tests/rp_backends.py), never the library on another route alone.  Every route
the bindings must follow is driven: host oracles and the device transcript kernels, the device entry points, culprit search (bisection and
CULPRITS = 1), the two half-batches, status compaction on the host and in HBM, shards and verify_each's chunks.

Small example shapes only (32bit, rec_test, bin_test); tables forced with COMB_MIN = 1 and kept small with COMB_BITS = 6."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import test_gpu_prove_device as PD
from bulletproofspp_amd import capi
from bulletproofspp_amd import encoding as E
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import array_to_point, load_test_library
from rp_backends import OracleBackend

pytestmark = pytest.mark.gpu

TAG = b"bound test"
SEED = hashlib.sha256(b"bound seed").digest()
NAMES = ["32bit", "rec_test", "bin_test"]          # inner-product flavour; typed, negative minimum, norm-linear; binary
VALID, INVALID = 0, 1
OK, OUT_OF_RANGE = 0, 3
ERR_ARG = -1
FILL = 0xA5
B3 = [bytes(range(32)), b"\xff" * 32, hashlib.sha256(b"a random binding").digest()]
ROUTES = ["no_table", "host_oracle", "device_oracle"]
_HOST_SETUPS, _REFS = {}, {}


def _bindings(n, label=b""):
    return [hashlib.sha256(b"binding %s %d" % (label, j)).digest() for j in range(n)]


def _mod(st):
    return BRP if isinstance(st, BRP.SetupBRP) else RP


def _nat(gpu, name, route="host_oracle", tag=TAG, **options):
    """a handle of an example under `tag`: no_table — the host-algebra routes of a handle without its comb table; host_oracle — the table in place,
    small batches hash on host cores; device_oracle — HOST_ORACLE_MAX = 0: k_rp_hash / k_rpp_hash hash every batch"""
    st = PD._setup(gpu, name)
    nat = (BRP.NativeBinaryRangeProofs if isinstance(st, BRP.SetupBRP) else RP.NativeRangeProofs)(gpu, st, oracle_tag=tag)
    if route != "no_table":
        nat.set_option("comb_min", 1)
    nat.set_option("comb_bits", PD.BITS)
    if route == "device_oracle":
        nat.set_option("host_oracle_max", 0)
    for k, v in options.items():
        nat.set_option(k, v)
    return nat


def _case(gpu, name, n, seed):
    st = PD._setup(gpu, name)
    return PD._inputs(name, st, n, seed), PD._prefixes(n, b"bound " + name.encode())


def _reference(oracle_lib, name, inputs, prefixes, bindings, tag=TAG):
    """the host protocol's proof of every (input, prefix, binding): [(files, challenges)], computed once per case and shared"""
    if name not in _HOST_SETUPS:
        schema = PD._schema(name)
        _HOST_SETUPS[name] = (BRP if schema.get("binary", False) else RP).setup_from_schema(OracleBackend(oracle_lib), schema)
    st = _HOST_SETUPS[name]
    mod = _mod(st)
    out = []
    for row, prefix, binding in zip(inputs, prefixes, bindings):
        key = (name, repr(row), prefix, binding, tag)
        if key not in _REFS:
            oracle = RP.sha256_oracle(tag + binding)
            wit = mod.witness(st, row)
            proof = mod.prove(st, wit, oracle, RP.hash_to_scalar(prefix))
            lead, es = mod.verifier_challenges(st, proof, RP.sha256_oracle(tag + binding))
            _REFS[key] = (E.encode_proof(2 if mod is BRP else 4, proof), (list(lead), list(es)))
        out.append(_REFS[key])
    return [f for f, _ in out], [c for _, c in out]


def _device_prove(nat, inputs, prefixes, bindings, status=False):
    """bppp_rp_prove_bound_device on uploaded arrays, the outputs prefilled: (files, statuses or None)"""
    gpu = nat.gpu
    with PD._DeviceCall(nat, inputs, prefixes) as call:
        d = call.d
        gpu.upload(d["cf"], np.full(call.cf.nbytes, FILL, dtype=np.uint8))
        gpu.upload(d["pf"], np.full(call.pf.nbytes, FILL, dtype=np.uint8))
        args = (call.B, d["amt"], 0 if call.binary else d["typ"], d["bld"], d["pre"], call.plen, d["cf"], d["pf"])
        st = nat.prove_batch_status_device(*args, bindings=bindings) if status else nat.prove_batch_device(*args, bindings=bindings)
        files = nat._prove_files(call.B, gpu.download(d["cf"], call.cf.shape, np.uint8), gpu.download(d["pf"], call.pf.shape, np.uint8))
    return files, (None if st is None else [int(s) for s in st])


class _Uploaded:
    """files (and bindings) in HBM for the _device verifiers"""

    def __init__(self, gpu, files, bindings=None):
        self.gpu, self.B = gpu, len(files)
        up = lambda raw: gpu.to_device(np.frombuffer(raw + b"\0" * (-len(raw) % 16) or bytes(16), dtype=np.uint8))
        self.dc, self.dp = up(b"".join(c for c, _ in files)), up(b"".join(p for _, p in files))
        self.db = up(b"".join(bindings)) if bindings is not None else 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in (self.dc, self.dp, self.db):
            if p:
                self.gpu.free(p)


def _raw_verify(nat, fn, lead, B, tail=()):
    """fn(handle, B, *lead, *tail, seed, &accept, status, challenges, combined_xy) -> (rc, accept, statuses, challenge words, point words)"""
    acc = C.c_int(-1)
    status = np.full(max(B, 1), 77, dtype=np.uint32)
    chal = np.zeros((max(B, 1) * nat.shape["challenges_per_proof"], 4), dtype=np.uint64)
    xy = np.zeros(8, dtype=np.uint64)
    sd = np.frombuffer(SEED, dtype=np.uint8)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    rc = fn(nat.h, B, *lead, *tail, vp(sd), C.byref(acc), vp(status), vp(chal), vp(xy))
    return rc, acc.value, [int(s) for s in status[:B]], chal.tobytes(), xy


def _split(files):
    return [c for c, _ in files], [p for _, p in files]


# ----------------------------------------------------------------------------- 1. prover bytes
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_prover_bytes_equal_the_host_protocol(gpu, oracle_lib, name, route):
    inputs, prefixes = _case(gpu, name, 3, 1)
    want, _ = _reference(oracle_lib, name, inputs, prefixes, B3)
    nat = _nat(gpu, name, route)
    try:
        assert nat.prove_batch(inputs, prefixes, bindings=B3) == want
        assert (nat.comb_info()["points"] == 0) == (route == "no_table")
        assert nat.prove_batch(inputs, prefixes, bindings=np.frombuffer(b"".join(B3), dtype=np.uint8).reshape(3, 32)) == want
        files, _ = _device_prove(nat, inputs, prefixes, B3)
        assert files == want
        files, statuses = _device_prove(nat, inputs, prefixes, B3, status=True)
        assert files == want and statuses == [OK] * 3
        got, statuses = nat.prove_batch_status(inputs, prefixes, bindings=B3)
        assert got == want and statuses == [OK] * 3
        unbound = nat.prove_batch(inputs, prefixes)
        assert all(u != w for u, w in zip(unbound, want)) and [u[0] for u in unbound] == [w[0] for w in want]      # other proofs, the same commitments
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 2. the handle law
@pytest.mark.parametrize("name", NAMES)
def test_a_handle_with_the_binding_in_its_tag_proves_the_same_bytes(gpu, oracle_lib, name):
    inputs, prefixes = _case(gpu, name, 3, 1)
    want, _ = _reference(oracle_lib, name, inputs, prefixes, B3)
    for b in (1, 2):                                                # 32 x ff, and the random one
        assert 0 not in B3[b]                                       # (a C string carries no zero byte: the law is stated for bindings without one)
        nat = _nat(gpu, name, "host_oracle", tag=TAG + B3[b])
        try:
            assert nat.prove_batch([inputs[b]], [prefixes[b]]) == [want[b]]
            assert nat.verify_batch([want[b][0]], [want[b][1]], SEED)
            assert not nat.verify_batch([want[0][0]], [want[0][1]], SEED)
        finally:
            nat.close()


# ----------------------------------------------------------------------------- 3. verifier
@pytest.mark.parametrize("route", ["host_oracle", "device_oracle"])
@pytest.mark.parametrize("name", NAMES)
def test_verifier(gpu, oracle_lib, name, route):
    inputs, prefixes = _case(gpu, name, 3, 1)
    files, chals = _reference(oracle_lib, name, inputs, prefixes, B3)
    coms, prfs = _split(files)
    swapped = [B3[2], B3[1], B3[0]]
    nat = _nat(gpu, name, route)
    try:
        ok, status, chs = nat.verify_batch(coms, prfs, SEED, want_status=True, want_challenges=True, bindings=B3)
        assert ok and status == [VALID] * 3
        for b in range(3):
            assert (list(chs[b][0]), list(chs[b][1])) == chals[b], b
        with _Uploaded(gpu, files, B3) as up, _Uploaded(gpu, files, swapped) as up_sw:
            ok, status, chs_d = nat.verify_batch_device(3, up.dc, up.dp, SEED, want_status=True, want_challenges=True, bindings=up.db)      # bindings in HBM
            assert ok and status == [VALID] * 3 and chs_d == chs
            for culprits in (0, 1):
                nat.set_option("culprits", culprits)
                ok, status, _ = nat.verify_batch(coms, prfs, SEED, want_status=True, bindings=swapped)
                assert not ok and status == [INVALID, VALID, INVALID], culprits
                ok, status, _ = nat.verify_batch_device(3, up.dc, up.dp, SEED, want_status=True, bindings=up_sw.db)
                assert not ok and status == [INVALID, VALID, INVALID], culprits
                ok, status, _ = nat.verify_batch(coms, prfs, SEED, want_status=True)                 # bindings = NULL
                assert not ok and status == [INVALID] * 3, culprits
            nat.set_option("culprits", 0)
        # unbound proofs under bindings = NULL: the unbound verifier's answers, word for word
        plain = nat.prove_batch(inputs, prefixes)
        lib = gpu.lib
        with _Uploaded(gpu, plain) as up:
            vp = C.c_void_p
            a = _raw_verify(nat, lib.bppp_rp_verify_bound_device, (0, vp(up.dc), vp(up.dp), None, None), 3)
            b_ = _raw_verify(nat, lib.bppp_rp_verify_batch_pub_device, (vp(up.dc), vp(up.dp), None), 3)
            assert a[0] == 0 and a[1] == 1 and a[2] == [VALID] * 3
            assert a[:4] == b_[:4] and a[4].tobytes() == b_[4].tobytes()
        cb, pb = (np.frombuffer(b"".join(x), dtype=np.uint8) for x in _split(plain))
        a = _raw_verify(nat, lib.bppp_rp_verify_bound, (C.c_void_p(cb.ctypes.data), C.c_void_p(pb.ctypes.data), None, None), 3)
        assert a[:4] == b_[:4] and a[4].tobytes() == b_[4].tobytes()
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 4. workgroup straddle
def test_seventy_proofs_straddle_the_hash_workgroups(gpu, oracle_lib):
    """HOST_ORACLE_MAX = 0 and 70 proofs: in k_rp_hash / k_rpp_hash g = h * batch + b puts two hash kinds and proofs past 64 into one workgroup —
    the smallest batch at which a wrong (b, h) header index shows"""
    B = 70
    inputs, prefixes = _case(gpu, "32bit", B, 4)
    bindings = _bindings(B, b"straddle")
    assert len(set(bindings)) == B
    want, _ = _reference(oracle_lib, "32bit", inputs, prefixes, bindings)
    coms, prfs = _split(want)
    nat = _nat(gpu, "32bit", "device_oracle")
    try:
        assert nat.prove_batch(inputs, prefixes, bindings=bindings) == want
        files, _ = _device_prove(nat, inputs, prefixes, bindings)
        assert files == want
        ok, status, _ = nat.verify_batch(coms, prfs, SEED, want_status=True, bindings=bindings)
        assert ok and status == [VALID] * B
        flipped = list(bindings)
        flipped[64] = bytes([flipped[64][0] ^ 1]) + flipped[64][1:]
        for culprits in (0, 1):
            nat.set_option("culprits", culprits)
            ok, status, _ = nat.verify_batch(coms, prfs, SEED, want_status=True, bindings=flipped)
            assert not ok and status == [INVALID if b == 64 else VALID for b in range(B)], culprits
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 5. verify_each_bound
@pytest.mark.parametrize("route", ["host_oracle", "device_oracle"])
@pytest.mark.parametrize("name", NAMES)
def test_verify_each(gpu, oracle_lib, name, route):
    inputs, prefixes = _case(gpu, name, 3, 1)
    files, _ = _reference(oracle_lib, name, inputs, prefixes, B3)
    coms, prfs = _split(files)
    swapped = [B3[2], B3[1], B3[0]]
    nat = _nat(gpu, name, route)
    try:
        status, pts = nat.verify_each(coms, prfs, want_points=True, bindings=B3)
        assert status == [VALID] * 3 and pts == [None] * 3                        # proof_xy all zero
        status, pts = nat.verify_each(coms, prfs, want_points=True, bindings=swapped)
        assert status == [INVALID, VALID, INVALID] and pts[1] is None and pts[0] is not None and pts[2] is not None
        assert nat.verify_each(coms, prfs) == [INVALID] * 3
        with _Uploaded(gpu, files, swapped) as up:
            assert nat.verify_each_device(3, up.dc, up.dp, want_points=True, bindings=up.db) == (status, pts)
            assert nat.verify_each_device(3, up.dc, up.dp, bindings=B3) == [VALID] * 3
    finally:
        nat.close()


def test_verify_each_in_two_chunks(gpu, oracle_lib):
    """chunks of 8 over 11 proofs (the test hook of test_gpu_verify_each.py): the second chunk starts at its own binding"""
    B = 11
    inputs, prefixes = _case(gpu, "32bit", B, 4)
    bindings = _bindings(B, b"straddle")
    files, _ = _reference(oracle_lib, "32bit", inputs, prefixes, bindings)
    coms, prfs = _split(files)
    nat = _nat(gpu, "32bit", "device_oracle")
    try:
        assert load_test_library().bppp_test_rp_set_each_chunk(nat.h, 8) == 0
        assert nat.verify_each(coms, prfs, bindings=bindings) == [VALID] * B
        wrong = list(bindings)
        wrong[9] = bindings[1]
        assert nat.verify_each(coms, prfs, bindings=wrong) == [INVALID if b == 9 else VALID for b in range(B)]
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 6. shards
@pytest.mark.parametrize("name", NAMES)
def test_shard_points_add_up(gpu, oracle_lib, name):
    """[0, 3) at offset 0 and [3, 5) at offset 3, each rank with the bindings of its own proofs: index_offset moves the weights, never the bindings.
    With every binding right all three points are the identity; with proofs 1 and 4 under wrong bindings they are not, and still add up."""
    B = 5
    inputs, prefixes = _case(gpu, name, B, 6)
    bindings = _bindings(B, b"shard")
    files, _ = _reference(oracle_lib, name, inputs, prefixes, bindings)
    wrong = list(bindings)
    wrong[1], wrong[4] = bindings[4], bindings[1]
    nat = _nat(gpu, name, "device_oracle")
    vp = C.c_void_p
    try:
        for bs, good in ((bindings, True), (wrong, False)):
            with _Uploaded(gpu, files, bs) as whole, _Uploaded(gpu, files[:3], bs[:3]) as lo, _Uploaded(gpu, files[3:], bs[3:]) as hi:
                fn = gpu.lib.bppp_rp_verify_bound_device
                rc, acc, _, _, xy = _raw_verify(nat, fn, (0, vp(whole.dc), vp(whole.dp), None, vp(whole.db)), 5)
                rc0, acc0, _, _, xy0 = _raw_verify(nat, fn, (0, vp(lo.dc), vp(lo.dp), None, vp(lo.db)), 3)
                rc1, acc1, _, _, xy1 = _raw_verify(nat, fn, (3, vp(hi.dc), vp(hi.dp), None, vp(hi.db)), 2)
            assert (rc, rc0, rc1) == (0, 0, 0) and (acc, acc0, acc1) == ((1, 1, 1) if good else (0, 0, 0))
            assert (array_to_point(xy) is None) == good and (array_to_point(xy0) is None) == good and (array_to_point(xy1) is None) == good
            assert gpu.sum_points(np.stack([xy0, xy1])) == array_to_point(xy)
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 7. the two half-batches
@pytest.mark.parametrize("route", ["host_oracle", "device_oracle"])
@pytest.mark.parametrize("name", NAMES)
def test_split_batch(gpu, oracle_lib, monkeypatch, name, route):
    monkeypatch.setenv("BPPP_RP_SPLIT_MIN_BINARY", "2")            # a binary handle takes its split threshold when it is created
    B = 5
    inputs, prefixes = _case(gpu, name, B, 6)
    bindings = _bindings(B, b"shard")
    want, _ = _reference(oracle_lib, name, inputs, prefixes, bindings)
    nat = _nat(gpu, name, route, split_min=2)
    monkeypatch.delenv("BPPP_RP_SPLIT_MIN_BINARY")
    whole = _nat(gpu, name, route, split_min=2**40)
    try:
        assert whole.prove_batch(inputs, prefixes, bindings=bindings) == want          # unsplit (builds the table)
        assert nat.prove_batch(inputs[:1], prefixes[:1], bindings=bindings[:1]) == want[:1]      # (the table before the split routes are asked for)
        assert nat.prove_batch(inputs, prefixes, bindings=bindings) == want            # [0, 3) here, [3, 5) on the twin handle
        files, _ = _device_prove(nat, inputs, prefixes, bindings)
        assert files == want
    finally:
        nat.close()
        whole.close()


# ----------------------------------------------------------------------------- 8. status compaction
def _out_of_range(name, row):
    """the witness with its first range at its upper end, balanced where the schema balances: refused as OUT_OF_RANGE"""
    if name == "rec_test":
        in2 = row[2][0]
        return [(2**64, 15, row[0][2]), (2**64 - 1 - in2, 15, row[1][2]), row[2]]
    if name == "bin_test":
        in1 = row[1][0]
        return [(2**64, row[0][1]), row[1], (2**64 - 2 - in1, row[2][1])]
    return [(2**32, 0, row[0][2])]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_status_compaction_keeps_each_proofs_binding(gpu, oracle_lib, name, route):
    B = 5
    inputs, prefixes = _case(gpu, name, B, 6)
    bindings = _bindings(B, b"shard")
    want, _ = _reference(oracle_lib, name, inputs, prefixes, bindings)
    for b in (1, 3):
        inputs[b] = _out_of_range(name, inputs[b])
    nat = _nat(gpu, name, route)
    zero = (bytes(nat.shape["coms_bytes"]), bytes(nat.shape["proof_bytes"]))
    expect = [OK, OUT_OF_RANGE, OK, OUT_OF_RANGE, OK]
    try:
        if route != "no_table":
            nat.prove_batch(inputs[:1], prefixes[:1])                                  # the table: the device variant runs as a stream of kernels
        files, statuses = nat.prove_batch_status(inputs, prefixes, bindings=bindings)
        assert statuses == expect and [f if f is not None else zero for f in files] == [want[b] if expect[b] == OK else zero for b in range(B)]
        files, statuses = _device_prove(nat, inputs, prefixes, bindings, status=True)
        assert statuses == expect and files == [want[b] if expect[b] == OK else zero for b in range(B)]
        with pytest.raises(capi.BpppError, match="proof [13]: "):                      # proof_status == NULL: a refused witness fails the call
            nat.prove_batch(inputs, prefixes, bindings=bindings)
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 9. errors
def test_errors(gpu, oracle_lib):
    inputs, prefixes = _case(gpu, "32bit", 3, 1)
    files, _ = _reference(oracle_lib, "32bit", inputs, prefixes, B3)
    coms, prfs = _split(files)
    lib = gpu.lib
    vp = lambda a: C.c_void_p(a.ctypes.data)
    long_tag = b"t" * 40
    nat = _nat(gpu, "32bit", "host_oracle", tag=long_tag)
    try:
        plain = nat.prove_batch(inputs, prefixes)                                      # unbound calls on a 40-byte tag keep working
        assert nat.verify_batch(*_split(plain), SEED) and nat.verify_each(*_split(plain)) == [VALID] * 3
        for call in (lambda: nat.prove_batch(inputs, prefixes, bindings=B3), lambda: nat.prove_batch_status(inputs, prefixes, bindings=B3),
                     lambda: nat.verify_batch(coms, prfs, SEED, bindings=B3), lambda: nat.verify_each(coms, prfs, bindings=B3)):
            with pytest.raises(capi.BpppError, match="oracle tag too long for per-proof bindings"):
                call()
        cb, pb = (np.frombuffer(b"".join(x), dtype=np.uint8) for x in _split(plain))
        bd = np.frombuffer(b"".join(B3), dtype=np.uint8)
        sd = np.frombuffer(SEED, dtype=np.uint8)
        acc = C.c_int(-1)
        assert lib.bppp_rp_verify_bound(nat.h, 3, vp(cb), vp(pb), None, vp(bd), vp(sd), C.byref(acc), None, None, None) == ERR_ARG
        assert b"tag too long" in lib.bppp_last_error(gpu.h)
        assert lib.bppp_rp_verify_bound(nat.h, 3, vp(cb), vp(pb), None, None, vp(sd), C.byref(acc), None, None, None) == 0 and acc.value == 1
    finally:
        nat.close()
    nat = _nat(gpu, "32bit", "host_oracle")
    try:
        bd = np.frombuffer(b"".join(B3), dtype=np.uint8)
        sd = np.frombuffer(SEED, dtype=np.uint8)
        acc, status = C.c_int(-1), np.zeros(3, dtype=np.uint32)
        # NULL files with a non-empty batch
        assert lib.bppp_rp_verify_bound(nat.h, 3, None, None, None, vp(bd), vp(sd), C.byref(acc), None, None, None) == ERR_ARG
        assert lib.bppp_rp_verify_bound_device(nat.h, 3, 0, None, None, None, vp(bd), vp(sd), C.byref(acc), None, None, None) == ERR_ARG
        assert lib.bppp_rp_verify_each_bound(nat.h, 3, None, None, None, vp(bd), vp(status), None) == ERR_ARG
        assert lib.bppp_rp_verify_each_bound_device(nat.h, 3, None, None, None, vp(bd), vp(status), None) == ERR_ARG
        assert lib.bppp_rp_prove_bound(nat.h, 3, None, None, None, None, vp(bd), None, 0, None, None, None) == ERR_ARG
        assert lib.bppp_rp_prove_bound_device(nat.h, 3, None, None, None, None, vp(bd), None, 0, None, None, vp(status)) == ERR_ARG
        # an empty batch
        acc = C.c_int(-1)
        assert lib.bppp_rp_verify_bound(nat.h, 0, None, None, None, None, None, C.byref(acc), None, None, None) == 0 and acc.value == 1
        assert lib.bppp_rp_verify_bound_device(nat.h, 0, 0, None, None, None, None, None, C.byref(acc), None, None, None) == 0
        assert lib.bppp_rp_verify_each_bound(nat.h, 0, None, None, None, None, vp(status), None) == 0
        assert lib.bppp_rp_verify_each_bound_device(nat.h, 0, None, None, None, None, vp(status), None) == 0
        assert lib.bppp_rp_prove_bound(nat.h, 0, None, None, None, None, None, None, 0, None, None, None) == 0
        assert lib.bppp_rp_prove_bound_device(nat.h, 0, None, None, None, None, None, None, 0, None, None, None) == 0
        assert nat.prove_batch([], [], bindings=[]) == [] and nat.prove_batch_status([], [], bindings=[]) == ([], [])
    finally:
        nat.close()
