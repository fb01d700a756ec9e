"""bppp_rp_prove_batch_device: range proofs from amounts, types and blindings in HBM to encoded files in HBM.  The files must equal, byte for
byte, what bppp_rp_prove_batch_pub writes for the same inputs on the same handle — on the device stream (witness kernel -> the provers' stream of
kernels -> encoding kernel) and on the slow path (routes without a device stream: download, host-buffer route, upload) — and a refused witness
must give the host entry point's return code and message.

Tables are forced with COMB_MIN = 1 and kept small with COMB_BITS = 6: megabytes, not gigabytes."""
import ctypes as C
import hashlib
import json
import os
import random

import numpy as np
import pytest

import pyoracle as O
import bulletproofspp_amd as b_
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import scalars_to_array
from test_rangeproof import EXAMPLES

pytestmark = pytest.mark.gpu

SEED = hashlib.sha256(b"prove device seed").digest()
N = O.N
BITS = 6
VALID, INVALID = 0, 1
ERR_ARG = -1
NAMES = ["32bit", "64bit", "32by64", "64by64", "96by64", "128by64", "rec_test", "bin_test"]
_SETUPS = {}


# ----------------------------------------------------------------------------- setups, witnesses, the two entry points side by side
def _schema(name):
    return json.load(open(os.path.join(EXAMPLES, name, "schema.json")))


def _setup(gpu, name, flavour=None):
    key = (name, flavour)
    if key not in _SETUPS:
        schema = _schema(name)
        if flavour is not None:
            schema["argument"] = flavour
        mod = BRP if schema.get("binary", False) else RP
        _SETUPS[key] = mod.setup_from_schema(RP.GpuBackend(gpu), schema)
    return _SETUPS[key]


def _native(gpu, st, table=True, **options):
    nat = (BRP.NativeBinaryRangeProofs if isinstance(st, BRP.SetupBRP) else RP.NativeRangeProofs)(gpu, st)
    if table:
        nat.set_option("comb_min", 1)
    nat.set_option("comb_bits", BITS)
    for k, v in options.items():
        nat.set_option(k, v)
    return nat


def _inputs(name, st, n, seed):
    """n witnesses of an example with random in-range amounts, the first proofs at the ends of the ranges (lo, hi - 1) as far as the
    schema's balance allows: rec_test (typed: 1 + in1 + in2 = out) cannot put in1 at hi - 1 = 2^66 - 2 under an output below 2^64 — that end is
    the witness-kernel test's; bin_test (conserved: 2 + in1 + in2 = out) has assumed inputs, which take whatever the output needs"""
    rnd = random.Random("%s %d" % (name, seed))
    bl = lambda: rnd.randrange(N)
    out = []
    for j in range(n):
        if name == "rec_test":
            lo1 = st.rds[1].lo
            in2 = 19 if j == 2 else rnd.randrange(19, 625)
            in1 = lo1 if j in (0, 2) else 2**64 - 2 - in2 if j == 1 else rnd.randrange(lo1, 2**63)      # j = 1: the output at 2^64 - 1, j = 2: at 0
            out.append([(1 + in1 + in2, 15, bl()), (in1, 15, bl()), (in2, 15, bl())])
        elif name == "bin_test":
            o = [3, 2**64 - 1][j] if j < 2 else rnd.randrange(3, 2**64)
            in1 = rnd.randrange(0, o - 2 + 1)
            out.append([(o, bl()), (in1, bl()), (o - 2 - in1, bl())])
        else:
            row = []
            for i, rd in enumerate(st.rds):
                v = rd.lo if j == 0 else rd.hi - 1 if j == 1 else rnd.randrange(rd.lo, rd.hi) if (i + j) % 3 else rnd.randrange(rd.lo, rd.lo + 70000)
                row.append((v, 0, bl()))
            out.append(row)
    return out


def _prefixes(n, tag=b""):
    return [b"prove device rnd %s %04d" % (tag, j) for j in range(n)]


class _DeviceCall:
    """the arrays of one prove call, on the host and uploaded: `amt`, `typ`, `bld` may be edited before `upload`.  alloc: another allocator than the
    handle's context (tests/guard_arena.py); the two file buffers then have coms_bytes and proof_bytes a proof and not a byte more"""

    def __init__(self, nat, inputs, prefixes, public_amounts=None, alloc=None):
        self.nat, self.gpu, self.B, self.slack = nat, alloc or nat.gpu, len(inputs), 0 if alloc else 16
        self.amt, self.typ, self.bld, self.pre, self.plen, self.cf, self.pf = nat._prove_arrays(nat._prove_rows(inputs), prefixes)
        self.amt, self.typ, self.bld = self.amt.copy(), self.typ.copy(), self.bld.copy()
        self.pub = None if public_amounts is None else nat._public_words(public_amounts, self.B)
        self.binary = isinstance(nat, BRP.NativeBinaryRangeProofs)
        self.d = {}

    def __enter__(self):
        g = self.gpu
        self.d = {"amt": g.to_device(self.amt), "typ": g.to_device(self.typ), "bld": g.to_device(self.bld), "pre": g.to_device(self.pre),
                  "cf": g.alloc(self.cf.nbytes + self.slack), "pf": g.alloc(self.pf.nbytes + self.slack), "pub": g.to_device(self.pub) if self.pub is not None else 0}
        return self

    def __exit__(self, *exc):
        for p in self.d.values():
            if p:
                self.gpu.free(p)

    def device_args(self):
        d = self.d
        vp = C.c_void_p
        return (self.nat.h, self.B, vp(d["amt"]), vp(0 if self.binary else d["typ"]), vp(d["bld"]), vp(d["pub"]), vp(d["pre"]), self.plen, vp(d["cf"]), vp(d["pf"]))

    def host_args(self):
        vp = lambda a: C.c_void_p(a.ctypes.data)
        return (self.nat.h, self.B, vp(self.amt), vp(self.typ), vp(self.bld), vp(self.pub) if self.pub is not None else None, vp(self.pre), self.plen,
                vp(self.cf), vp(self.pf))

    def raw_device(self):
        rc = self.gpu.lib.bppp_rp_prove_batch_device(*self.device_args())
        return rc, self.gpu.lib.bppp_last_error(self.gpu.h).decode() if rc else ""

    def raw_host(self):
        rc = self.gpu.lib.bppp_rp_prove_batch_pub(*self.host_args())
        return rc, self.gpu.lib.bppp_last_error(self.gpu.h).decode() if rc else ""

    def device_files(self):
        d = self.d
        self.nat.prove_batch_device(self.B, d["amt"], 0 if self.binary else d["typ"], d["bld"], d["pre"], self.plen, d["cf"], d["pf"], d["pub"])
        return self.nat._prove_files(self.B, self.gpu.download(d["cf"], self.cf.shape, np.uint8), self.gpu.download(d["pf"], self.pf.shape, np.uint8))


def _device_files(nat, inputs, prefixes, public_amounts=None):
    with _DeviceCall(nat, inputs, prefixes, public_amounts) as call:
        return call.device_files()


# ----------------------------------------------------------------------------- 1. bytes, every example, both flavours, every route
NPROOFS = 24


@pytest.mark.parametrize("flavour", ["NL", "IP"])
@pytest.mark.parametrize("name", NAMES)
def test_files_equal_the_host_entry_points(gpu, monkeypatch, name, flavour):
    monkeypatch.setenv("BPPP_RP_SPLIT_MIN_BINARY", "2")            # a binary handle takes its split threshold when it is created
    st = _setup(gpu, name, flavour)
    inputs, prefixes = _inputs(name, st, NPROOFS, 1), _prefixes(NPROOFS, name.encode())
    nat = _native(gpu, st, table=False, split_min=2**40)
    try:
        assert nat.comb_info()["points"] == 0
        few = 5                                                      # no table yet: the slow path (host algebra for most shapes)
        want_few = nat.prove_batch(inputs[:few], prefixes[:few])
        assert _device_files(nat, inputs[:few], prefixes[:few]) == want_few
        assert nat.comb_info()["points"] == 0
        nat.set_option("comb_min", 1)
        want = nat.prove_batch(inputs, prefixes)                     # builds the table: one stream of kernels from here on
        assert nat.comb_info()["points"] > 0 and want[:few] == want_few
        assert _device_files(nat, inputs, prefixes) == want          # host oracle (at most 64 proofs)
        nat.set_option("host_oracle_max", 0)
        assert _device_files(nat, inputs, prefixes) == want          # device oracle
        nat.set_option("host_oracle_max", 2**64 - 1)
        nat.set_option("split_min", 2)
        assert _device_files(nat, inputs, prefixes) == want          # the twin handle takes the second half
        nat.set_option("split_min", 2**40)
        nat.set_option("host_algebra", 1)
        assert _device_files(nat, inputs[:few], prefixes[:few]) == want_few
    finally:
        nat.close()


def test_files_over_a_donors_shared_table(gpu):
    donor = _native(gpu, _setup(gpu, "64by64"))
    own, borrower = _native(gpu, _setup(gpu, "32by64")), _native(gpu, _setup(gpu, "32by64"))
    try:
        borrower.share_comb(donor)
        assert borrower.comb_info() == donor.comb_info() and borrower.comb_info()["points"] > 1 + borrower.shape["lin_len"] + borrower.shape["norm_len"]
        inputs, prefixes = _inputs("32by64", own.st, 9, 2), _prefixes(9, b"donor")
        want = own.prove_batch(inputs, prefixes)
        assert borrower.prove_batch(inputs, prefixes) == want
        assert _device_files(borrower, inputs, prefixes) == want
        assert borrower.comb_info() == donor.comb_info()
    finally:
        for h in (own, borrower, donor):
            h.close()


# ----------------------------------------------------------------------------- 2. per-proof public amounts in HBM
PTS = O.hash_points(b"prove device", 120)
FEE_TYPE = 7


def _typed_setup(gpu, fee=0):
    """2 inputs + 2 outputs of 32 bits (inline, base 4, with a bit) and one public fee, an OUTPUT: in1 + in2 = out1 + out2 + fee"""
    rds = [RP.make_range_data(4, 0, 2**32, False, False, False), RP.make_range_data(4, 0, 2**32, False, False, False),
           RP.make_range_data(4, 0, 2**32, False, True, False), RP.make_range_data(4, 0, 2**32, False, True, False)]
    return RP.setup(RP.GpuBackend(gpu), PTS, True, [(True, FEE_TYPE, fee)], rds, "NL")


def _typed_inputs(fees, seed):
    rnd = random.Random(seed)
    out = []
    for fee in fees:
        total = fee + rnd.randrange(2**31)
        i1 = rnd.randrange(max(total - (2**32 - 1), 0), min(total, 2**32 - 1) + 1)
        o1 = rnd.randrange(total - fee + 1)
        out.append([(i1, FEE_TYPE, rnd.randrange(N)), (total - i1, FEE_TYPE, rnd.randrange(N)), (o1, FEE_TYPE, rnd.randrange(N)),
                    (total - fee - o1, FEE_TYPE, rnd.randrange(N))])
    return out


def _binary_schema(net):
    return dict(_schema("bin_test"), public=[{"amount": net, "isOutput": False}])


def _binary_inputs(nets, seed):
    """bin_test's shape: one output in [3, 2^64), two assumed inputs; net + in1 + in2 - out = 0"""
    rnd = random.Random(seed)
    out = []
    for net in nets:
        i1, i2 = rnd.randrange(100, 1000), rnd.randrange(100, 1000)
        out.append([(net + i1 + i2, rnd.randrange(N)), (i1, rnd.randrange(N)), (i2, rnd.randrange(N))])
    return out


@pytest.fixture(scope="module")
def typed(gpu):
    nat = _native(gpu, _typed_setup(gpu))
    nat.prove_batch(_typed_inputs([0], 0), _prefixes(1, b"warm"))       # the table is in place from here on
    assert nat.comb_info()["points"] > 0
    yield nat
    nat.close()


@pytest.fixture(scope="module")
def binary(gpu):
    nat = _native(gpu, BRP.setup_from_schema(RP.GpuBackend(gpu), _binary_schema(0)))
    nat.prove_batch(_binary_inputs([0], 0), _prefixes(1, b"warm"))
    assert nat.comb_info()["points"] > 0
    yield nat
    nat.close()


def test_public_amounts_typed(typed):
    fees = [0, 5, 5, 2**32 + 7, 17, 0, 1234567, 3]
    inputs, prefixes = _typed_inputs(fees, 1), _prefixes(len(fees), b"fee")
    pubs = [[f] for f in fees]
    want = typed.prove_batch(inputs, prefixes, public_amounts=pubs)
    assert _device_files(typed, inputs, prefixes, pubs) == want
    typed.set_option("split_min", 2)
    try:
        assert _device_files(typed, inputs, prefixes, pubs) == want       # each half takes its slice of the amounts
    finally:
        typed.set_option("split_min", 4096)
    zero = _typed_inputs([0] * 4, 2)
    assert _device_files(typed, zero, prefixes[:4]) == typed.prove_batch(zero, prefixes[:4]) == typed.prove_batch(zero, prefixes[:4], public_amounts=[[0]] * 4)


def test_public_amounts_binary(binary):
    nets = [2, 2, -22, 0, 2**40, 7, -1]
    inputs, prefixes = _binary_inputs(nets, 9), _prefixes(len(nets), b"net")
    want = binary.prove_batch(inputs, prefixes, public_amounts=nets)
    assert _device_files(binary, inputs, prefixes, nets) == want
    zero = _binary_inputs([0] * 3, 4)
    assert _device_files(binary, zero, prefixes[:3]) == binary.prove_batch(zero, prefixes[:3])


# ----------------------------------------------------------------------------- 3. the witness kernel alone
def _witness_device(nat, inputs, public_amounts=None):
    """bppp_test_rp_witness_device: (in_sc [B][nr][3] ints, dig, mul, mss as lists per proof, status)"""
    gpu, tlib = nat.gpu, capi.load_test_library()
    B, nr = len(inputs), len(nat.st.rds)
    binary = isinstance(nat, BRP.NativeBinaryRangeProofs)
    nlen, nmss = nat.shape["norm_len"], 0 if binary else nat.shape["lin_len"] - 6
    if binary:
        nlen = sum(len(rd.base_coeffs) for rd in nat.st.rds if not rd.is_assumed)       # the bits of the live positions
    call = _DeviceCall(nat, inputs, _prefixes(B), public_amounts)
    if binary and public_amounts is not None:
        call.pub = scalars_to_array([v % N for v in public_amounts])        # the hook takes canonical scalars, as the kernel does
    with call:
        in_sc = np.zeros((B * nr * 3, 4), dtype=np.uint64)
        dig, mul = np.full(B * nlen + 1, 77, dtype=np.uint32), np.full(B * nlen + 1, 77, dtype=np.uint32)
        mss, status = np.full(B * nmss + 1, 77, dtype=np.uint32), np.full(B, 77, dtype=np.uint32)
        d = call.d
        vp = lambda a: C.c_void_p(a.ctypes.data)
        rc = tlib.bppp_test_rp_witness_device(nat.h, B, C.c_void_p(d["amt"]), C.c_void_p(d["typ"]), C.c_void_p(d["bld"]), C.c_void_p(d["pub"]), vp(in_sc), vp(dig),
                                              vp(mul), vp(mss), vp(status))
        assert rc == 0, gpu.lib.bppp_last_error(gpu.h)
    flat = capi.array_to_scalars(in_sc)
    sc = [[tuple(flat[(b * nr + i) * 3:(b * nr + i) * 3 + 3]) for i in range(nr)] for b in range(B)]
    cut = lambda a, n: [[int(x) for x in a[b * n:(b + 1) * n]] for b in range(B)]
    return sc, cut(dig, nlen), cut(mul, nlen), cut(mss, nmss), [int(s) for s in status]


def _witness_host(st, row):
    """what make_witness hands the device prover for one proof, from the Python restatement: in_sc, dig (0 at typing positions), mul, mss"""
    w = RP.witness(st, row)
    ds, ms = RP.get_ds_ms(w.ph1s)
    ds = [0 if p[0] == "typing" else d for p, d in zip(w.ph1s, ds)]
    return [tuple(t) for t in w.inputs], ds, ms, [m for _, mm in w.base_mss for m in mm]


def _digits_abi(rd, v):
    lib = capi.load_library()
    arr = (capi.RpRange * 1)()
    arr[0].base = rd.base
    arr[0].flags = (capi.RP_SHARED if rd.is_shared else 0) | (capi.RP_OUTPUT if rd.is_output else 0)
    arr[0].min[:] = [int(x) for x in capi.int_to_limbs(rd.lo % 2**256)]
    arr[0].max[:] = [int(x) for x in capi.int_to_limbs(rd.hi % 2**256)]
    out, nd, hb = np.zeros(300, dtype=np.uint32), C.c_size_t(0), C.c_int(0)
    amt = capi.int_to_limbs(v % 2**256)
    assert lib.bppp_rp_digits(C.cast(arr, C.c_void_p), amt.ctypes.data, out.ctypes.data, 300, C.byref(nd), C.byref(hb)) == 0
    return [int(x) for x in out[:nd.value]]


def test_witness_kernel_matches_the_host_witness(gpu):
    """an untyped setup (amounts are free): a base-1000 shared range; shared base 16 over a width above 2^100 with a negative minimum; shared
    base 256 over a width close to 2^255 (the host's bisection over a 256 x 32-bit product); inline base 4 with a bit ([0, 2^32]); inline base 4 with a
    negative minimum; an assumed range (no digits)"""
    mk = RP.make_range_data
    rds = [mk(1000, 0, 10**9, True, True), mk(16, -5, 2**100 + 12345, True, False), mk(256, -2**254, 2**254 - 3, True, False), mk(4, 0, 2**32 + 1, False, True),
           mk(4, -20, 44, False, False), mk(5, 1, 625, False, False, True), mk(16, 0, 2**64, True, True)]
    assert all(rd is not None for rd in rds) and rds[3].has_bit
    nrm = sum(len(rd.base_coeffs) for rd in rds)
    lin = 6 + 999 + 15 + 255 + 1
    st = RP.setup(RP.GpuBackend(gpu), RP.basis_points(b"witness kernel", 2 + nrm + lin + 2), False, [], rds, "NL")
    nat = _native(gpu, st, table=False)
    try:
        assert nat.shape["lin_len"] == st.lin_len and any(rd.has_bit and rd.is_shared for rd in rds) == (2 in st.m_bases)
        rnd = random.Random(3)
        rows = []
        for j in range(40):
            row = []
            for i, rd in enumerate(rds):
                if rd.is_assumed:
                    v = rnd.choice([0, -7, 2**200, rnd.randrange(1, 625)])      # assumed: never checked, never decomposed
                elif j == 0:
                    v = rd.lo
                elif j == 1:
                    v = rd.hi - 1
                elif j == 2:
                    v = rd.lo + 1
                elif j % 4 == 3:
                    v = rd.lo + rnd.randrange(min(rd.hi - rd.lo, 2**16))         # small remainders: the host's 64-bit path
                elif j % 4 == 0:
                    v = rd.hi - 1 - rnd.randrange(min(rd.hi - rd.lo, 2**70))
                else:
                    v = rnd.randrange(rd.lo, rd.hi)
                row.append((v, rnd.randrange(N), rnd.randrange(N)))
            rows.append(row)
        sc, dig, mul, mss, status = _witness_device(nat, rows)
        assert status == [0] * len(rows)
        for b, row in enumerate(rows):
            want_sc, want_dig, want_mul, want_mss = _witness_host(st, row)
            assert sc[b] == want_sc, b
            assert dig[b] == want_dig and mul[b] == want_mul and mss[b] == want_mss, b
            for i, rd in enumerate(rds):                                        # ... and the library's own host digits
                if not rd.is_assumed:
                    p0 = sum(len(r.base_coeffs) for r in rds[:i])
                    assert dig[b][p0:p0 + len(rd.base_coeffs)] == _digits_abi(rd, row[i][0]), (b, i)
    finally:
        nat.close()


def test_witness_kernel_typed_and_binary(gpu, typed, binary):
    st = _setup(gpu, "rec_test")
    nat = _native(gpu, st, table=False)
    try:
        rows = _inputs("rec_test", st, 12, 5)
        sc, dig, mul, mss, status = _witness_device(nat, rows)
        assert status == [0] * 12
        for b, row in enumerate(rows):
            assert (sc[b], dig[b], mul[b], mss[b]) == _witness_host(st, row), b
    finally:
        nat.close()
    fees = [0, 9, 2**32 + 1, 77]
    rows = _typed_inputs(fees, 6)
    sc, dig, mul, mss, status = _witness_device(typed, rows, [[f] for f in fees])
    assert status == [0] * 4
    for b, row in enumerate(rows):
        assert (sc[b], dig[b], mul[b], mss[b]) == _witness_host(_typed_setup(gpu, fees[b]), row), b
    assert _witness_device(typed, rows)[4] == [0, 2, 2, 2]                      # the handle's own fee (0): the others do not balance
    nets = [2, -22, 2**40]
    rows = _binary_inputs(nets, 7) + [[(3, 5), (0, 6), (3 - 2**40, 7)], [(2**64 - 1, 5), (2**64 - 1 - 2**40, 6), (0, 7)]]
    nets += [2**40, 2**40]
    sc, bits, _, _, status = _witness_device(binary, rows, nets)
    assert status == [0] * len(rows)
    for b, row in enumerate(rows):
        stb = BRP.setup_from_schema(RP.GpuBackend(gpu), _binary_schema(nets[b]))
        assert sc[b] == [(v % N, bl % N, 0) for v, bl in row], b
        assert bits[b] == [int(d) for d in BRP.witness(stb, row)[1]] and len(bits[b]) == len(stb.rds[0].base_coeffs), b


# ----------------------------------------------------------------------------- 4. errors: the host entry point's code and text
def _both(call):
    with call:
        host, dev = call.raw_host(), call.raw_device()
    return host, dev


def _set(arr, index, value):
    arr[index] = capi.int_to_limbs(value % 2**256)


def test_refused_witnesses_typed(typed):
    B = 8
    fees = [3] * B
    inputs, prefixes, pubs = _typed_inputs(fees, 11), _prefixes(B, b"err"), [[3]] * B
    nr = 4

    def case(edit, expect):
        call = _DeviceCall(typed, inputs, prefixes, pubs)
        edit(call)
        host, dev = _both(call)
        assert host[0] == ERR_ARG and dev == host and expect in dev[1], (host, dev)
        return dev

    def below(c, b=3):                       # in1 = -1, in2 takes the difference: the types still balance, the range check refuses
        tot = inputs[b][0][0] + inputs[b][1][0]
        _set(c.amt, b * nr, -1); _set(c.amt, b * nr + 1, tot + 1)

    def at_max(c, b=5):                      # out1 = 2^32 = hi
        tot = inputs[b][2][0] + inputs[b][3][0]
        _set(c.amt, b * nr + 2, 2**32); _set(c.amt, b * nr + 3, tot - 2**32)

    case(below, "proof 3: value outside its range")
    case(at_max, "proof 5: value outside its range")
    case(lambda c: _set(c.bld, 6 * nr + 1, N), "proof 6: type / blinding not canonical")
    case(lambda c: _set(c.typ, 0, N + 5), "proof 0: type / blinding not canonical")
    case(lambda c: _set(c.amt, 2 * nr + 2, inputs[2][2][0] + 1), "proof 2: amounts of some type do not balance")
    case(lambda c: _set(c.amt, 7 * nr, 2**32 + 5), "proof 7: amounts of some type do not balance")          # out of range AND unbalanced: balance first
    # two refused proofs: the lowest-numbered one, with the host's text for that proof alone
    alone = case(lambda c: below(c, 2), "proof 2: value outside its range")
    call = _DeviceCall(typed, inputs, prefixes, pubs)
    below(call, 2); _set(call.amt, 6 * nr + 2, inputs[6][2][0] + 1)
    with call:
        assert call.raw_device() == alone
    typed.set_option("split_min", 2)         # a refused proof of the second half keeps its index in the whole batch
    try:
        case(lambda c: at_max(c, 6), "proof 6: value outside its range")
    finally:
        typed.set_option("split_min", 4096)


def test_refused_witnesses_binary(binary):
    nets = [2, 7, 0, 2, 2, 2]
    inputs, prefixes = _binary_inputs(nets, 12), _prefixes(len(nets), b"berr")
    nr = 3

    def case(edit, expect):
        call = _DeviceCall(binary, inputs, prefixes, nets)
        edit(call)
        host, dev = _both(call)
        assert host[0] == ERR_ARG and dev == host and expect in dev[1], (host, dev)

    def below(c):                            # the output at 2 < 3 with the inputs (assumed: unchecked) keeping the balance
        _set(c.amt, 4 * nr, 2); _set(c.amt, 4 * nr + 1, 0); _set(c.amt, 4 * nr + 2, 0)
    case(below, "proof 4: value outside its range")
    case(lambda c: _set(c.amt, 1 * nr, 2**64), "proof 1: value outside its range")
    case(lambda c: _set(c.bld, 2 * nr + 2, N), "proof 2: blinding is not canonical")
    case(lambda c: _set(c.amt, 3 * nr + 1, inputs[3][1][0] + 1), "proof 3: a binary witness needs a conserved schema")


def test_argument_errors(gpu, typed):
    inputs, prefixes = _typed_inputs([0, 0], 13), _prefixes(2, b"arg")
    lib = gpu.lib
    with _DeviceCall(typed, inputs, prefixes) as call:
        dev, host = list(call.device_args()), list(call.host_args())

        def both(i, value):
            a, h = list(dev), list(host)
            a[i] = h[i] = value
            rd, ed = lib.bppp_rp_prove_batch_device(*a), lib.bppp_last_error(gpu.h)
            rh, eh = lib.bppp_rp_prove_batch_pub(*h), lib.bppp_last_error(gpu.h)
            assert rd == rh == ERR_ARG and ed == eh, (i, ed, eh)
        for i in (2, 3, 4, 6, 8, 9):                                  # NULL buffers with a non-empty batch
            both(i, None)
        both(1, 2**20)
        both(7, 4097)
        assert lib.bppp_rp_prove_batch_device(*([dev[0], 0] + [None] * 5 + [0, None, None])) == 0     # an empty batch
    # public amounts on a handle whose public_count is 0; a non-canonical typed amount
    rds = [RP.make_range_data(4, 0, 2**32, False, False, False)]
    untyped = _native(gpu, RP.setup(RP.GpuBackend(gpu), PTS, False, [], rds, "NL"))
    try:
        with _DeviceCall(untyped, [[(5, 0, 1)]], _prefixes(1)) as call:
            call.pub = scalars_to_array([0])
            call.d["pub"] = gpu.to_device(call.pub)
            host, dev = call.raw_host(), call.raw_device()
            assert host[0] == ERR_ARG and dev == host and "no public amounts" in dev[1]
    finally:
        untyped.close()
    with _DeviceCall(typed, inputs, prefixes, [[0], [0]]) as call:
        call.pub[1] = capi.int_to_limbs(N)
        gpu.upload(call.d["pub"], call.pub)
        host, dev = call.raw_host(), call.raw_device()
        assert host[0] == ERR_ARG and dev == host and "proof 1: public amount 0 is not canonical" in dev[1]
    # a closed context: destroyed straight through the C ABI (Bppp.close() would close the handle with it)
    ctx2 = b_.Bppp(0)
    nat2 = _native(ctx2, _typed_setup(ctx2))
    with _DeviceCall(nat2, inputs, prefixes) as call:
        h, ctx2.h = ctx2.h, None
        lib.bppp_ctx_destroy(h)
        assert lib.bppp_rp_prove_batch_device(*call.device_args()) == ERR_ARG == lib.bppp_rp_prove_batch_pub(*call.host_args())
        call.d = {}                                                   # the buffers went with the context's last reference or stay until exit
    nat2.close()


# ----------------------------------------------------------------------------- 5. prove into HBM, verify from the same pointers
def test_prove_then_verify_without_a_host_copy(typed):
    B = 16
    fees = [b * 11 for b in range(B)]
    inputs, prefixes, pubs = _typed_inputs(fees, 14), _prefixes(B, b"pipe"), [[f] for f in fees]
    with _DeviceCall(typed, inputs, prefixes, pubs) as call:
        d = call.d
        typed.prove_batch_device(B, d["amt"], d["typ"], d["bld"], d["pre"], call.plen, d["cf"], d["pf"], d["pub"])
        ok, status, _ = typed.verify_batch_device(B, d["cf"], d["pf"], SEED, want_status=True, public_amounts=d["pub"])
        assert ok and status == [VALID] * B
        off = 9 * typed.shape["proof_bytes"] + 5
        byte = typed.gpu.download(d["pf"] + off, (1,), np.uint8)
        typed.gpu.upload(d["pf"] + off, byte ^ np.uint8(1))
        ok, status, _ = typed.verify_batch_device(B, d["cf"], d["pf"], SEED, want_status=True, public_amounts=d["pub"])
        assert not ok and status == [INVALID if b == 9 else VALID for b in range(B)]


# ----------------------------------------------------------------------------- 6. the comb table is built at the same point
@pytest.mark.parametrize("device", [False, True])
def test_table_is_built_at_comb_min(gpu, device):
    nat = _native(gpu, _typed_setup(gpu), table=False, comb_min=64)
    try:
        inputs, prefixes = _typed_inputs([0] * 40, 15), _prefixes(40, b"book")
        run = (lambda: _device_files(nat, inputs, prefixes)) if device else (lambda: nat.prove_batch(inputs, prefixes))
        first = run()
        assert nat.comb_info()["points"] == 0
        assert run() == first
        assert nat.comb_info()["points"] > 0
    finally:
        nat.close()
