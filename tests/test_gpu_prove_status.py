"""bppp_rp_prove_batch_status / bppp_rp_prove_batch_status_device: the batch prover with a verdict per proof.  A witness the counterparts
(bppp_rp_prove_batch_pub, bppp_rp_prove_batch_device) refuse no longer fails the call: its status says why, its two files are zero bytes, and
every other proof is proved in the same pass — byte for byte the files the counterpart writes for the accepted proofs alone, on the host-buffer
routes, on the device stream (witness kernel -> index lists -> witness kernel over the accepted -> prover -> encoding through dst_index ->
zeroing kernel) and on the device entry point's slow path.

Every output buffer is filled with 0xA5 before a call, so a file that was never written shows.  Tables are forced with COMB_MIN = 1 and kept
small with COMB_BITS = 6, as in test_gpu_prove_device.py (whose helpers this file imports)."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_prove_device as PD
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from test_gpu_prove_device import ERR_ARG, N, NAMES, SEED, VALID, _binary_inputs, _binary_schema, _inputs, _native, _prefixes, _set, _setup, _typed_inputs, _typed_setup
from test_gpu_prove_device import binary, typed      # noqa: F401 (module-scoped fixtures: a typed fee handle and a binary one with their tables in place)

pytestmark = pytest.mark.gpu

OK, NOT_CANONICAL, UNBALANCED, OUT_OF_RANGE, BIN_NOT_CANONICAL, BIN_UNBALANCED = 0, 1, 2, 3, 4, 5
FILL = 0xA5


def _text(gpu, status):
    return gpu.lib.bppp_rp_witness_status_text(status).decode()


class _StatusCall(PD._DeviceCall):
    """one call's arrays (test_gpu_prove_device._DeviceCall) through the two *_status entry points: (rc, message, statuses, files)"""

    def _result(self, rc, status, cf, pf):
        err = self.gpu.lib.bppp_last_error(self.gpu.h).decode() if rc else ""
        return rc, err, [int(s) for s in status], self.nat._prove_files(self.B, cf, pf)

    def status_host(self):
        self.cf[:] = FILL
        self.pf[:] = FILL
        status = np.full(self.B, 77, dtype=np.uint32)
        rc = self.gpu.lib.bppp_rp_prove_batch_status(*self.host_args(), C.c_void_p(status.ctypes.data))
        return self._result(rc, status, self.cf, self.pf)

    def _fill_device(self):
        self.gpu.upload(self.d["cf"], np.full(self.cf.nbytes, FILL, dtype=np.uint8))
        self.gpu.upload(self.d["pf"], np.full(self.pf.nbytes, FILL, dtype=np.uint8))

    def _device_out(self):
        return self.gpu.download(self.d["cf"], self.cf.shape, np.uint8), self.gpu.download(self.d["pf"], self.pf.shape, np.uint8)

    def status_device(self):
        self._fill_device()
        status = np.full(self.B, 77, dtype=np.uint32)
        rc = self.gpu.lib.bppp_rp_prove_batch_status_device(*self.device_args(), C.c_void_p(status.ctypes.data))
        return self._result(rc, status, *self._device_out())

    def rows(self, arr, idx):
        return np.ascontiguousarray(arr.reshape(self.B, -1)[idx])

    def host_subset(self, idx):
        """bppp_rp_prove_batch_pub on proofs idx of this call's (edited) arrays alone, in that order: (rc, message, files)"""
        nat, n = self.nat, len(idx)
        amt, typ, bld, pre = (self.rows(a, idx) for a in (self.amt, self.typ, self.bld, self.pre))
        pub = self.rows(self.pub, idx) if self.pub is not None else None
        cf, pf = np.full(n * nat.shape["coms_bytes"], FILL, dtype=np.uint8), np.full(n * nat.shape["proof_bytes"], FILL, dtype=np.uint8)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        rc = self.gpu.lib.bppp_rp_prove_batch_pub(nat.h, n, vp(amt), vp(typ), vp(bld), vp(pub) if pub is not None else None, vp(pre), self.plen, vp(cf), vp(pf))
        return rc, self.gpu.lib.bppp_last_error(self.gpu.h).decode() if rc else "", nat._prove_files(n, cf, pf)


def _zero_pair(nat):
    return bytes(nat.shape["coms_bytes"]), bytes(nat.shape["proof_bytes"])


def _check_mixed(call, expect, pubs=None, verify=True):
    """both entry points on one batch: the expected verdicts; host and device agree byte for byte; a refused proof alone fails the counterpart with
    the verdict's text and its files are zero; the accepted files are the counterpart's on the accepted proofs alone, and verify"""
    nat, gpu = call.nat, call.gpu
    with call:
        rc_h, err_h, st_h, files_h = call.status_host()
        rc_d, err_d, st_d, files_d = call.status_device()
    print("statuses host %s device %s" % (st_h, st_d))
    assert rc_h == 0 and rc_d == 0, (err_h, err_d)
    assert st_h == expect and st_d == expect
    assert files_h == files_d
    accepted = [b for b in range(call.B) if expect[b] == OK]
    for b in range(call.B):
        if expect[b] != OK:
            rc, err, _ = call.host_subset([b])
            assert rc == ERR_ARG and "proof 0: " + _text(gpu, expect[b]) in err, (b, err)
            assert files_h[b] == _zero_pair(nat), b
    if accepted:
        rc, err, want = call.host_subset(accepted)
        assert rc == 0, err
        assert [files_h[b] for b in accepted] == want
        if verify:
            sub = None if pubs is None else [pubs[b] for b in accepted]
            assert nat.verify_batch([c for c, _ in want], [p for _, p in want], SEED, public_amounts=sub)
    refused = [b for b in range(call.B) if expect[b] != OK]
    if refused and verify:
        zc, zp = _zero_pair(nat)
        assert nat.verify_each([zc], [zp], public_amounts=None if pubs is None else [pubs[refused[0]]])[0] != VALID
    return files_h


# ----------------------------------------------------------------------------- 1, 2. no refusal: the counterparts' bytes on every route
NPROOFS = 6


@pytest.mark.parametrize("name", NAMES)
def test_all_good_equals_the_counterparts(gpu, name):
    st = _setup(gpu, name)
    inputs, prefixes = _inputs(name, st, NPROOFS, 21), _prefixes(NPROOFS, b"st " + name.encode())
    nat = _native(gpu, st)
    try:
        want = nat.prove_batch(inputs, prefixes)
        assert nat.comb_info()["points"] > 0
        files, statuses = nat.prove_batch_status(inputs, prefixes)
        assert statuses == [OK] * NPROOFS and files == want
        with PD._DeviceCall(nat, inputs, prefixes) as call:            # the device stream
            assert call.device_files() == want
            d = call.d
            gpu.upload(d["cf"], np.full(call.cf.nbytes, FILL, dtype=np.uint8))
            gpu.upload(d["pf"], np.full(call.pf.nbytes, FILL, dtype=np.uint8))
            status = nat.prove_batch_status_device(call.B, d["amt"], 0 if call.binary else d["typ"], d["bld"], d["pre"], call.plen, d["cf"], d["pf"])
            assert status.dtype == np.uint32 and list(status) == [OK] * NPROOFS
            assert nat._prove_files(call.B, gpu.download(d["cf"], call.cf.shape, np.uint8), gpu.download(d["pf"], call.pf.shape, np.uint8)) == want
    finally:
        nat.close()


@pytest.mark.parametrize("route", ["no_table", "host_algebra", "fold_points"])
@pytest.mark.parametrize("name", ["64by64", "rec_test", "bin_test"])
def test_slow_path_of_the_device_variant(gpu, name, route):
    """routes without a device stream: the inputs come down, the host-buffer route proves, the files go up — without and with a refusal"""
    st = _setup(gpu, name)
    B = 5
    inputs, prefixes = _inputs(name, st, B, 22), _prefixes(B, b"slow")
    nat = _native(gpu, st, table=route != "no_table")
    try:
        if route != "no_table":                                         # the table first (HOST_ALGEBRA alone would never build it), then the option
            nat.prove_batch(inputs[:1], prefixes[:1])
            nat.set_option(route, 1)
        with _StatusCall(nat, inputs, prefixes) as call:
            want = call.device_files()
            assert (nat.comb_info()["points"] == 0) == (route == "no_table")
            rc, err, status, files = call.status_device()
            assert rc == 0 and status == [OK] * B and files == want, err
            assert call.status_host()[2:] == (status, files)
        nr = len(st.rds)
        call = _StatusCall(nat, inputs, prefixes)
        _set(call.amt, 1 * nr, 2**64)                                   # range 0 of proof 1 at hi
        if name == "rec_test":                                          # ... with in1 keeping the types' balance, which is checked before the ranges
            _set(call.amt, 1 * nr + 1, 2**64 - 1 - inputs[1][2][0])
        _set(call.bld, 4 * nr, N)
        expect = [OK, OUT_OF_RANGE, OK, OK, BIN_NOT_CANONICAL if call.binary else NOT_CANONICAL]
        files = _check_mixed(call, expect, verify=False)
        assert [files[b] for b in (0, 2, 3)] == [want[b] for b in (0, 2, 3)]
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 3. mixed batches, typed-reciprocal handles
def test_mixed_batch_rec_test(gpu):
    """rec_test (typed: 1 + in1 + in2 = out, all of type 15; out in [0, 2^64), in1 in [-20, 2^66 - 1), in2 assumed): every reason, the first and
    the last proof among the refused"""
    st = _setup(gpu, "rec_test")
    B, nr = 14, 3
    inputs, prefixes = _inputs("rec_test", st, B, 31), _prefixes(B, b"mix rec")
    nat = _native(gpu, st)
    try:
        call = _StatusCall(nat, inputs, prefixes)
        in2 = lambda b: inputs[b][2][0]
        _set(call.amt, 0 * nr + 1, -21); _set(call.amt, 0 * nr, 1 - 21 + in2(0))            # in1 below its range, the output keeps the balance
        _set(call.amt, 3 * nr, 2**64); _set(call.amt, 3 * nr + 1, 2**64 - 1 - in2(3))        # the output at hi, balanced
        _set(call.amt, 5 * nr, inputs[5][0][0] + 1)                                          # unbalanced, in range
        _set(call.amt, 6 * nr + 1, -21)                                                      # out of range AND unbalanced: the balance is checked first
        _set(call.bld, 8 * nr + 1, N)
        _set(call.typ, 9 * nr + 2, N + 15)
        _set(call.amt, 13 * nr, -1); _set(call.amt, 13 * nr + 1, -7); _set(call.amt, 13 * nr + 2, 5)      # the output below 0: 1 - 7 + 5 = -1
        expect = [OK] * B
        expect[0] = expect[3] = expect[13] = OUT_OF_RANGE
        expect[5] = expect[6] = UNBALANCED
        expect[8] = expect[9] = NOT_CANONICAL
        _check_mixed(call, expect)
    finally:
        nat.close()


def test_mixed_batch_64by64(gpu):
    """64by64 is an UNTYPED setup (64 shared ranges [0, 2^64), no public values): its witness check has no balance, so UNBALANCED cannot occur
    here (rec_test and the typed fee setup below cover it); every other reason does, with the lowest code winning"""
    st = _setup(gpu, "64by64")
    B, nr = 14, 64
    inputs, prefixes = _inputs("64by64", st, B, 32), _prefixes(B, b"mix 64")
    nat = _native(gpu, st)
    try:
        call = _StatusCall(nat, inputs, prefixes)
        _set(call.amt, 0 * nr + 5, -1)
        _set(call.amt, 2 * nr + 63, 2**64)
        _set(call.bld, 4 * nr, N)
        _set(call.typ, 7 * nr + 1, N + 3)
        _set(call.amt, 9 * nr + 2, 2**64 + 1); _set(call.bld, 9 * nr + 40, 2**256 - 1)      # out of range AND not canonical: canonical is checked first
        _set(call.amt, 13 * nr + 63, 2**64 + 5)
        expect = [OK] * B
        expect[0] = expect[2] = expect[13] = OUT_OF_RANGE
        expect[4] = expect[7] = expect[9] = NOT_CANONICAL
        _check_mixed(call, expect)
        nat.set_option("host_oracle_max", 0)                              # the device oracle on the compacted batch
        _check_mixed(call, expect, verify=False)
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 4. binary; per-proof public amounts
def test_mixed_batch_bin_test(gpu):
    """bin_test (conserved: 2 + in1 + in2 = out; out in [3, 2^64), the inputs assumed): the first offending range decides, then the balance"""
    st = _setup(gpu, "bin_test")
    B, nr = 12, 3
    inputs, prefixes = _inputs("bin_test", st, B, 41), _prefixes(B, b"mix bin")
    nat = _native(gpu, st)
    try:
        call = _StatusCall(nat, inputs, prefixes)
        _set(call.amt, 0 * nr, 2); _set(call.amt, 0 * nr + 1, 0); _set(call.amt, 0 * nr + 2, 0)      # the output below 3, balanced
        _set(call.bld, 4 * nr + 2, N)
        _set(call.amt, 6 * nr + 1, inputs[6][1][0] + 1)                                            # unbalanced
        _set(call.amt, 7 * nr, 2**64); _set(call.bld, 7 * nr + 2, N)                               # range 0 out of range comes before range 2's blinding
        _set(call.amt, 8 * nr, 2**64); _set(call.bld, 8 * nr, N + 1)                               # range 0: its blinding, then its bounds
        _set(call.amt, 11 * nr, 2**64); _set(call.amt, 11 * nr + 1, 2**64 - 2 - inputs[11][2][0])   # the output at hi, balanced
        expect = [OK] * B
        expect[0] = expect[7] = expect[11] = OUT_OF_RANGE
        expect[4] = expect[8] = BIN_NOT_CANONICAL
        expect[6] = BIN_UNBALANCED
        _check_mixed(call, expect)
    finally:
        nat.close()


def test_public_amounts_follow_their_proofs_typed(gpu, typed):
    """in1 + in2 = out1 + out2 + fee with one fee per proof: a fee balances its own proof and not its neighbour's; behind refused proofs the
    gathered public words must still be those of the proof in the slot — each accepted file equals the one a handle CREATED with that fee writes"""
    fees = [3, 3, 5, 0, 9, 2**32 + 7, 1, 4, 6, 8, 11, 12]
    B, nr = len(fees), 4
    inputs, prefixes = _typed_inputs(fees, 51), _prefixes(B, b"fee st")
    given = list(fees)
    given[1], given[2] = 5, 5                                   # proof 2 balances under 5, proof 1 (made for 3) does not
    given[7] = 6                                                # made for 4
    pubs = [[f] for f in given]
    call = _StatusCall(typed, inputs, prefixes, pubs)
    tot = inputs[0][0][0] + inputs[0][1][0]
    _set(call.amt, 0 * nr, -1); _set(call.amt, 0 * nr + 1, tot + 1)      # balanced, below its range
    _set(call.bld, (B - 1) * nr + 3, N)
    expect = [OK] * B
    expect[0], expect[1], expect[7], expect[B - 1] = OUT_OF_RANGE, UNBALANCED, UNBALANCED, NOT_CANONICAL
    files = _check_mixed(call, expect, pubs)
    for b in (2, 5, 10):
        own = _native(typed.gpu, _typed_setup(typed.gpu, fees[b]))
        try:
            assert own.prove_batch([inputs[b]], [prefixes[b]]) == [files[b]], b
        finally:
            own.close()
    typed.set_option("split_min", 2)                            # each half gathers its own slice of the amounts
    try:
        assert _check_mixed(call, expect, pubs, verify=False) == files
    finally:
        typed.set_option("split_min", 4096)


def test_public_amounts_follow_their_proofs_binary(gpu, binary):
    nets = [2, 7, 0, 2, -22, 2**40, 5, 5, 9]
    B, nr = len(nets), 3
    inputs, prefixes = _binary_inputs(nets, 52), _prefixes(B, b"net st")
    given = list(nets)
    given[0], given[3] = 7, 0                                   # made for 2: neither balances; proof 1 (made for 7) does
    call = _StatusCall(binary, inputs, prefixes, given)
    _set(call.bld, 6 * nr + 1, N)
    expect = [OK] * B
    expect[0] = expect[3] = BIN_UNBALANCED
    expect[6] = BIN_NOT_CANONICAL
    files = _check_mixed(call, expect, given)
    for b in (1, 4, 5, 8):
        own = _native(gpu, BRP.setup_from_schema(RP.GpuBackend(gpu), _binary_schema(nets[b])))
        try:
            assert own.prove_batch([inputs[b]], [prefixes[b]]) == [files[b]], b
        finally:
            own.close()


# ----------------------------------------------------------------------------- 5. two half-batches in flight
def _halves_cases(B):
    """the refused proofs of each case: in both halves, in the first only, in the second only, in neither"""
    half = (B + 1) // 2
    return [[1, half - 1, half, B - 1], [0, 2], [half + 1], []]


def test_two_halves_typed(gpu, typed):
    B, nr = 11, 4
    fees = [2] * B
    inputs, prefixes, pubs = _typed_inputs(fees, 61), _prefixes(B, b"halves"), [[2]] * B
    for refused in _halves_cases(B):
        call = _StatusCall(typed, inputs, prefixes, pubs)
        expect = [OK] * B
        for j, b in enumerate(refused):
            if j % 2:
                _set(call.amt, b * nr + 2, inputs[b][2][0] + 1); expect[b] = UNBALANCED
            else:
                _set(call.amt, b * nr + 2, 2**32); _set(call.amt, b * nr + 3, inputs[b][2][0] + inputs[b][3][0] - 2**32); expect[b] = OUT_OF_RANGE
        whole = _check_mixed(call, expect, pubs, verify=False)
        typed.set_option("split_min", 2)
        try:
            assert _check_mixed(call, expect, pubs, verify=False) == whole, refused       # statuses at whole-batch indices, the unsplit call's bytes
        finally:
            typed.set_option("split_min", 4096)


def test_two_halves_binary(gpu, monkeypatch):
    st = _setup(gpu, "bin_test")
    B, nr = 10, 3
    inputs, prefixes = _inputs("bin_test", st, B, 62), _prefixes(B, b"bhalves")
    whole_nat = _native(gpu, st)
    monkeypatch.setenv("BPPP_RP_SPLIT_MIN_BINARY", "2")            # a binary handle takes its split threshold when it is created
    split_nat = _native(gpu, st)
    try:
        for refused in _halves_cases(B):
            results = []
            for nat in (whole_nat, split_nat):
                call = _StatusCall(nat, inputs, prefixes)
                expect = [OK] * B
                for j, b in enumerate(refused):
                    if j % 2:
                        _set(call.amt, b * nr + 1, inputs[b][1][0] + 1); expect[b] = BIN_UNBALANCED
                    else:
                        _set(call.bld, b * nr, N); expect[b] = BIN_NOT_CANONICAL
                results.append(_check_mixed(call, expect, verify=False))
            assert results[0] == results[1], refused
    finally:
        whole_nat.close()
        split_nat.close()


# ----------------------------------------------------------------------------- 6. edges
def test_all_refused_and_the_table_bookkeeping(gpu):
    """every proof refused: BPPP_OK, zero files — and the decision to build the comb table, taken on the submitted batch before any witness is looked
    at, has built it, as a refused bppp_rp_prove_batch_pub call of that size does"""
    B, nr = 5, 4
    inputs, prefixes = _typed_inputs([0] * B, 71), _prefixes(B, b"none")
    nat = _native(gpu, _typed_setup(gpu), table=False, comb_min=B)
    try:
        call = _StatusCall(nat, inputs, prefixes)
        for b in range(B):
            _set(call.amt, b * nr, inputs[b][0][0] + 1 + b)
        with call:
            assert nat.comb_info()["points"] == 0
            rc, err, status, files = call.status_host()
            assert rc == 0 and status == [UNBALANCED] * B and files == [_zero_pair(nat)] * B, err
            assert nat.comb_info()["points"] > 0
            rc, err, status, files = call.status_device()          # the device stream with nothing to prove
            assert rc == 0 and status == [UNBALANCED] * B and files == [_zero_pair(nat)] * B, err
    finally:
        nat.close()


def test_batch_of_one(gpu, typed, binary):
    inputs, prefixes = _typed_inputs([4], 72), _prefixes(1, b"one")
    _check_mixed(_StatusCall(typed, inputs, prefixes, [[4]]), [OK], [[4]])
    _check_mixed(_StatusCall(typed, inputs, prefixes, [[5]]), [UNBALANCED], [[5]])
    inputs = _binary_inputs([3], 73)
    _check_mixed(_StatusCall(binary, inputs, prefixes, [3]), [OK], [3])
    call = _StatusCall(binary, inputs, prefixes, [3])
    _set(call.amt, 0, 2)
    _check_mixed(call, [OUT_OF_RANGE], [3])


def test_argument_errors_stay_call_level(gpu, typed):
    lib = gpu.lib
    inputs, prefixes = _typed_inputs([0, 0], 74), _prefixes(2, b"arg st")
    with _StatusCall(typed, inputs, prefixes) as call:
        status = np.full(2, 77, dtype=np.uint32)
        sp = C.c_void_p(status.ctypes.data)
        dev, host = list(call.device_args()), list(call.host_args())
        # an empty batch; a NULL proof_status
        assert lib.bppp_rp_prove_batch_status(*([host[0], 0] + [None] * 5 + [0, None, None, None])) == 0
        assert lib.bppp_rp_prove_batch_status_device(*([dev[0], 0] + [None] * 5 + [0, None, None, None])) == 0
        assert lib.bppp_rp_prove_batch_status(*(host + [None])) == ERR_ARG and b"proof_status" in lib.bppp_last_error(gpu.h)
        assert lib.bppp_rp_prove_batch_status_device(*(dev + [None])) == ERR_ARG and b"proof_status" in lib.bppp_last_error(gpu.h)

        def same_as_counterpart(i, value):
            a, h = list(dev), list(host)
            a[i] = h[i] = value
            for fn, ref, args in ((lib.bppp_rp_prove_batch_status_device, lib.bppp_rp_prove_batch_device, a), (lib.bppp_rp_prove_batch_status, lib.bppp_rp_prove_batch_pub, h)):
                want = (ref(*args), lib.bppp_last_error(gpu.h))
                assert want[0] == ERR_ARG and (fn(*(args + [sp])), lib.bppp_last_error(gpu.h)) == want, (i, want)
        for i in (2, 3, 4, 6, 8, 9):                                  # NULL buffers with a non-empty batch
            same_as_counterpart(i, None)
        same_as_counterpart(1, 2**20)
        same_as_counterpart(7, 4097)
    # a public amount that is not canonical: the counterpart's code and message, no verdicts
    with _StatusCall(typed, inputs, prefixes, [[0], [0]]) as call:
        call.pub[1] = capi.int_to_limbs(N)
        gpu.upload(call.d["pub"], call.pub)
        want_h, want_d = call.raw_host(), call.raw_device()
        assert want_h[0] == ERR_ARG and want_d == want_h and "proof 1: public amount 0 is not canonical" in want_h[1]
        assert call.status_host()[:2] == want_h and call.status_device()[:2] == want_d
    # a closed context
    import bulletproofspp_amd as b_
    ctx2 = b_.Bppp(0)
    nat2 = _native(ctx2, _typed_setup(ctx2))
    with _StatusCall(nat2, inputs, prefixes) as call:
        h, ctx2.h = ctx2.h, None
        lib.bppp_ctx_destroy(h)
        status = np.full(2, 77, dtype=np.uint32)
        sp = C.c_void_p(status.ctypes.data)
        assert lib.bppp_rp_prove_batch_status_device(*call.device_args(), sp) == ERR_ARG == lib.bppp_rp_prove_batch_status(*call.host_args(), sp)
        call.d = {}
    nat2.close()


# ----------------------------------------------------------------------------- 7. a larger batch on the device stream
def test_512_proofs_every_seventh_refused(gpu):
    st = _setup(gpu, "64by64")
    B, nr = 512, 64
    inputs, prefixes = _inputs("64by64", st, B, 81), _prefixes(B, b"big")
    nat = _native(gpu, st)
    try:
        accepted = [b for b in range(B) if b % 7]
        with PD._DeviceCall(nat, [inputs[b] for b in accepted], [prefixes[b] for b in accepted]) as sub:
            want = sub.device_files()                                 # bppp_rp_prove_batch_device on the accepted proofs alone
        assert nat.comb_info()["points"] > 0
        call = _StatusCall(nat, inputs, prefixes)
        for b in range(0, B, 7):
            _set(call.amt, b * nr + b % nr, 2**64)
        with call:
            rc, err, status, files = call.status_device()
        assert rc == 0, err
        assert status == [OK if b % 7 else OUT_OF_RANGE for b in range(B)]
        assert [files[b] for b in accepted] == want
        assert all(files[b] == _zero_pair(nat) for b in range(0, B, 7))
    finally:
        nat.close()
