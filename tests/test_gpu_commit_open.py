"""bppp_rp_commit_batch*, bppp_rp_open_each*, bppp_rp_open_batch*: commitments without a proof, and checking their openings.

The reference side is the host protocol code over the oracle backend (tests/rp_backends.py): C = v g + ty H0 + bl H1 by its commit (a binary
setup: v g + bl h0, scalarRPW'), encoding.encode_commitments for the files, its group law for the combined point — never the library under test.
References are computed once per setup for 65 rows and shared; smaller batches are prefixes of the same rows."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import capi, encoding
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from rp_backends import OracleBackend
from test_gpu_prove_device import _inputs
from test_rangeproof import EXAMPLES

pytestmark = pytest.mark.gpu

N = O.N
SEED = hashlib.sha256(b"commit open seed").digest()
ERR_ARG = -1
OK, MISMATCH, MALFORMED, NOT_CANONICAL = 0, 1, 2, 3
NINE = {"basisSeed": "test points", "ranges": [{"base": 9, "min": 0, "max": 4294967296, "isOutput": True, "count": 9}]}      # a sign field that straddles a byte
NAMES = ["32bit", "rec_test", "bin_test", "64by64", "nine"]
ROWS = 65                                    # one lane past a wavefront
_CACHE = {}


def _case(oracle_lib, name):
    """(setup, ROWS valid witnesses in prove_batch's shape, the same as (v, ty, bl) triples, reference points [ROWS][nranges], reference files)"""
    if name not in _CACHE:
        schema = NINE if name == "nine" else json.load(open(os.path.join(EXAMPLES, name, "schema.json")))
        binary = bool(schema.get("binary", False))
        st = (BRP if binary else RP).setup_from_schema(OracleBackend(oracle_lib), schema)
        inputs = _inputs("32bit" if name == "nine" else name, st, ROWS, 7)
        triples = [[(v, 0, bl) for v, bl in row] for row in inputs] if binary else inputs
        pts = [_ref_points(oracle_lib, st, row) for row in triples]
        _CACHE[name] = (st, inputs, triples, pts, [encoding.encode_commitments(row) for row in pts])
    return _CACHE[name]


def _ref_points(ec, st, triples):
    if isinstance(st, BRP.SetupBRP):
        return [ec.inner_product([(v % N, st.g), (bl % N, st.hs[0])]) for v, _, bl in triples]
    return [ec.inner_product([(v % N, st.g), (ty % N, st.hs[0]), (bl % N, st.hs[1])]) for v, ty, bl in triples]


def _native(gpu, st):
    return (BRP.NativeBinaryRangeProofs if isinstance(st, BRP.SetupBRP) else RP.NativeRangeProofs)(gpu, st)


@pytest.fixture(scope="module")
def handles(gpu, oracle_lib):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _native(gpu, _case(oracle_lib, name)[0])
        return made[name]
    yield get
    for nat in made.values():
        nat.close()


class _Dev:
    """the claimed arrays (and files) of one call in HBM; alloc: another allocator than the handle's context (tests/guard_arena.py)"""

    def __init__(self, nat, inputs, coms_files=None, alloc=None):
        self.nat, self.gpu, self.B = nat, alloc or nat.gpu, len(inputs)
        self.binary = isinstance(nat, BRP.NativeBinaryRangeProofs)
        amt, typ, bld = nat._claim_arrays(inputs)
        self.cb = nat.shape["coms_bytes"]
        files = np.frombuffer(b"".join(coms_files), dtype=np.uint8) if coms_files is not None else np.full(self.B * self.cb, 0xA5, dtype=np.uint8)
        g = self.gpu
        self.d = {"amt": g.to_device(amt), "typ": 0 if self.binary else g.to_device(typ), "bld": g.to_device(bld), "cf": g.to_device(files)}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.d.values():
            if p:
                self.gpu.free(p)

    def files(self):
        raw = self.gpu.download(self.d["cf"], (self.B * self.cb,), np.uint8)
        return [raw[b * self.cb:(b + 1) * self.cb].tobytes() for b in range(self.B)]

    def claims(self):
        return self.d["amt"], self.d["typ"], self.d["bld"]


# ----------------------------------------------------------------------------- 1. commit = reference = prover, host = device
@pytest.mark.parametrize("name", NAMES)
def test_commit_equals_reference_and_prover(gpu, oracle_lib, handles, name):
    st, inputs, _, _, want = _case(oracle_lib, name)
    nat = handles(name)
    for B in (1, 3, ROWS):
        files = nat.commit_batch(inputs[:B])
        assert files == want[:B], B
        with _Dev(nat, inputs[:B]) as dev:
            status = nat.commit_batch_device(B, *dev.claims(), dev.d["cf"], want_status=True)
            assert list(status) == [0] * B and dev.files() == want[:B], B
    proved = nat.prove_batch(inputs, [b"commit open rnd %04d" % b for b in range(ROWS)])
    assert [c for c, _ in proved] == want


# ----------------------------------------------------------------------------- 2. no witness is judged
def test_commit_needs_no_witness(gpu, oracle_lib, handles):
    st, inputs, _, _, _ = _case(oracle_lib, "rec_test")
    nat = handles("rec_test")
    rows = [list(inputs[0]), list(inputs[1]), list(inputs[2])]
    rows[0][0] = (2**200 + 5, 15, rows[0][0][2])                 # far outside [0, 2^64)
    rows[1][1] = (-(2**70), 15, rows[1][1][2])                   # below the negative minimum
    rows[2][2] = (rows[2][2][0] + 1, 15, rows[2][2][2])          # the types no longer balance
    with pytest.raises(capi.BpppError):
        nat.prove_batch(rows[2:], [b"unbalanced rnd 0"])
    files, status = nat.commit_batch(rows, want_status=True)
    assert status == [0, 0, 0]
    assert files == [encoding.encode_commitments(_ref_points(oracle_lib, st, row)) for row in rows]


# ----------------------------------------------------------------------------- 3. statuses, and the same inputs without a status array
@pytest.mark.parametrize("name", ["rec_test", "bin_test"])
def test_commit_statuses(gpu, oracle_lib, handles, name):
    st, inputs, _, _, want = _case(oracle_lib, name)
    nat = handles(name)
    binary = name == "bin_test"
    rows = [list(r) for r in inputs[:5]]
    rows[1][1] = (rows[1][1][0], N) if binary else (rows[1][1][0], N, rows[1][1][2])                      # binary: blinding = n; typed: type = n
    rows[3] = [(0, 0)] * len(rows[3]) if binary else [(0, 0, 0)] * len(rows[3])                          # every commitment of the row is infinity
    code = capi.RP_WIT_BIN_NOT_CANONICAL if binary else capi.RP_WIT_NOT_CANONICAL
    files, status = nat.commit_batch(rows, want_status=True)
    assert status == [0, code, 0, capi.RP_COMMIT_INFINITY, 0]
    assert files == [want[0], None, want[2], None, want[4]]
    with _Dev(nat, rows) as dev:
        dstatus = nat.commit_batch_device(5, *dev.claims(), dev.d["cf"], want_status=True)
        zero = bytes(nat.shape["coms_bytes"])
        assert list(dstatus) == status and dev.files() == [want[0], zero, want[2], zero, want[4]]
    with pytest.raises(capi.BpppError, match="proof 1: "):
        nat.commit_batch(rows)
    with pytest.raises(capi.BpppError, match="proof 1: .*infinity"):
        nat.commit_batch([rows[0], rows[3]])
    assert nat.commit_batch([rows[0], rows[2]]) == [want[0], want[2]]


# ----------------------------------------------------------------------------- 4. open_each
def _no_point_x(ec):
    x = 0
    while ec.lift_x(x) is not None:
        x += 1
    return x


def _flip_sign(file, i):
    f = bytearray(file)
    f[i >> 3] ^= 1 << (i & 7)
    return bytes(f)


def _set_x(file, nr, i, x):
    ns = (nr + 7) // 8
    return file[:ns + 32 * i] + encoding.put_field(x) + file[ns + 32 * (i + 1):]


def test_open_each(gpu, oracle_lib, handles):
    for name in ("rec_test", "nine", "bin_test"):
        st, inputs, _, _, want = _case(oracle_lib, name)
        nat, nr, binary = handles(name), len(st.rds), name == "bin_test"
        B = 5
        good = [[OK] * nr for _ in range(B)]
        assert nat.open_each(want[:B], inputs[:B]) == good
        with _Dev(nat, inputs[:B], want[:B]) as dev:
            assert nat.open_each_device(B, dev.d["cf"], *dev.claims()) == good

        def changed(b, i, f):
            rows = [list(r) for r in inputs[:B]]
            rows[b][i] = f(rows[b][i])
            return rows

        def only(b, i, code):
            out = [list(r) for r in good]
            out[b][i] = code
            return out
        b, i = 3, nr - 1
        bl_at = 1 if binary else 2
        edits = [lambda t: (t[0] + 1,) + t[1:], lambda t: t[:bl_at] + ((t[bl_at] + 1) % N,)]
        if not binary:
            edits.append(lambda t: (t[0], t[1] + 1, t[2]))
        for f in edits:
            assert nat.open_each(want[:B], changed(b, i, f)) == only(b, i, MISMATCH)
        files = list(want[:B])
        files[b] = _flip_sign(files[b], i)
        assert nat.open_each(files, inputs[:B]) == only(b, i, MISMATCH)
        files[b] = _set_x(want[b], nr, i, _no_point_x(oracle_lib))
        assert nat.open_each(files, inputs[:B]) == only(b, i, MALFORMED)
        assert nat.open_each(want[:B], changed(b, i, lambda t: t[:bl_at] + (N,))) == only(b, i, NOT_CANONICAL)
        if not binary:
                # the prover's reduction: an amount is a plain integer reduced mod n, so v and v + n are one amount.  Both must fit the 256-bit
                # two's-complement word the entry points take (v + n < 2^255), which leaves the most negative v: commit to v, open with v + n
                low = -2**255 + 5
                rows = changed(b, i, lambda t: (low, t[1], t[2]))
                committed = nat.commit_batch(rows)
                assert committed[b] == encoding.encode_commitments(_ref_points(oracle_lib, st, rows[b]))
                assert 0 < low + N < 2**255 and nat.open_each(committed, changed(b, i, lambda t: (low + N, t[1], t[2]))) == good


# ----------------------------------------------------------------------------- 5. open_batch
def _job_weight(nat, st, seed, offset, files, triples, b, i):
    nr = len(st.rds)
    ns = (nr + 7) // 8
    v, ty, bl = triples[b][i]
    return RP.open_weight(seed, (offset + b) * nr + i, files[b][ns + 32 * i:ns + 32 * (i + 1)], (files[b][i >> 3] >> (i & 7)) & 1, v % N, ty % N, bl % N)


@pytest.mark.parametrize("name,B", [("32bit", 3), ("64by64", ROWS), ("64by64", 129)])
def test_open_batch(gpu, oracle_lib, handles, name, B):
    """3 x 32bit and 65 x 64by64 (4160 + 3 terms) take the MSM's one-launch route for up to 8192 terms, 129 x 64by64 (8256 + 3) its general
    pipeline.  The 129 rows are the 65 reference rows followed by the first 64 of them again."""
    st, inputs, triples, _, want = _case(oracle_lib, name)
    nat, nr, ec = handles(name), len(st.rds), oracle_lib
    idx = [r % ROWS for r in range(B)]
    inputs, triples, files = [inputs[r] for r in idx], [triples[r] for r in idx], [want[r] for r in idx]
    acc, status, point = nat.open_batch(files, inputs, SEED, want_status=True, want_point=True)
    assert acc and status == [[OK] * nr] * B and point is None
    assert nat.open_batch(files, inputs) is True                                   # a fresh seed
    b, i = B - 1, nr - 1
    bad = [list(r) for r in inputs]
    bad[b][i] = (bad[b][i][0] + 1,) + tuple(bad[b][i][1:])
    bad_t = [list(r) for r in triples]
    bad_t[b][i] = (triples[b][i][0] + 1,) + tuple(triples[b][i][1:])
    acc, status, point = nat.open_batch(files, bad, SEED, want_status=True, want_point=True)
    # E = C - (v + 1) g - ty H0 - bl H1 = -g
    assert not acc and point == ec.mul((-_job_weight(nat, st, SEED, 0, files, bad_t, b, i)) % N, st.g)
    assert status == nat.open_each(files, bad) and status[b][i] == MISMATCH and sum(map(sum, status)) == MISMATCH
    seed2 = hashlib.sha256(SEED).digest()
    acc2, _, point2 = nat.open_batch(files, bad, seed2, want_point=True)
    assert not acc2 and point2 not in (None, point) and point2 == ec.mul((-_job_weight(nat, st, seed2, 0, files, bad_t, b, i)) % N, st.g)
    with _Dev(nat, bad, files) as dev:
        cf, claims = dev.d["cf"], dev.claims()
        acc0, st0, p0 = nat.open_batch_device(B, cf, *claims, seed=SEED, index_offset=0, want_status=True, want_point=True)
        assert (acc0, st0, p0) == (False, status, point)
        acc7, _, p7 = nat.open_batch_device(B, cf, *claims, seed=SEED, index_offset=7, want_point=True)
        assert not acc7 and p7 == ec.mul((-_job_weight(nat, st, SEED, 7, files, bad_t, b, i)) % N, st.g) and p7 != point
        if B > 33:                                                                 # two shards of one job
            w = nr * 8 * 4                                                         # bytes of a row of claims
            off = lambda p, rows, stride: p + rows * stride if p else 0
            a0, _, s0 = nat.open_batch_device(33, cf, *claims, seed=SEED, index_offset=0, want_point=True)
            a1, _, s1 = nat.open_batch_device(B - 33, off(cf, 33, dev.cb), off(claims[0], 33, w), off(claims[1], 33, w), off(claims[2], 33, w), seed=SEED,
                                              index_offset=33, want_point=True)
            assert a0 and s0 is None and not a1 and s1 == point                    # identity + the second shard's point
    with _Dev(nat, inputs, files) as dev:
        assert nat.open_batch_device(B, dev.d["cf"], *dev.claims(), seed=SEED, index_offset=2**40) is True
    # a malformed x and a non-canonical claim reject, with open_each's verdicts
    broken = list(files)
    broken[0] = _set_x(files[0], nr, 0, _no_point_x(ec))
    acc, status, _ = nat.open_batch(broken, inputs, SEED, want_status=True)
    assert not acc and status == nat.open_each(broken, inputs) and status[0][0] == MALFORMED
    claim_n = [list(r) for r in inputs]
    claim_n[0][0] = tuple(claim_n[0][0][:-1]) + (N,)
    acc, status, _ = nat.open_batch(files, claim_n, SEED, want_status=True)
    assert not acc and status == nat.open_each(files, claim_n) and status[0][0] == NOT_CANONICAL


def test_open_batch_binary(gpu, oracle_lib, handles):
    """a binary handle: C = v g + bl h0, the weight message carries a zero type"""
    st, inputs, triples, _, want = _case(oracle_lib, "bin_test")
    nat, nr, B = handles("bin_test"), len(st.rds), 4
    assert nat.open_batch(want[:B], inputs[:B], SEED) is True
    bad = [list(r) for r in inputs[:B]]
    bad[2][1] = (bad[2][1][0], (bad[2][1][1] + 1) % N)
    bad_t = [[(v, 0, bl) for v, bl in row] for row in bad]
    acc, status, point = nat.open_batch(want[:B], bad, SEED, want_status=True, want_point=True)
    assert not acc and status == nat.open_each(want[:B], bad) and status[2][1] == MISMATCH
    assert point == oracle_lib.mul((-_job_weight(nat, st, SEED, 0, want, bad_t, 2, 1)) % N, st.hs[0])     # E = -h0


# ----------------------------------------------------------------------------- 6. argument errors and the empty batch
def test_argument_errors_and_empty_batch(gpu, oracle_lib, handles):
    st, inputs, _, _, want = _case(oracle_lib, "rec_test")
    nat, lib = handles("rec_test"), gpu.lib
    amt, typ, bld = nat._claim_arrays(inputs[:2])
    cf = np.frombuffer(b"".join(want[:2]), dtype=np.uint8).copy()
    status, acc, sd = np.zeros(8, dtype=np.uint32), C.c_int(-1), np.frombuffer(SEED, dtype=np.uint8)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    h = nat.h
    # empty batches
    assert lib.bppp_rp_commit_batch(h, 0, None, None, None, None, None) == 0
    assert lib.bppp_rp_open_each(h, 0, None, None, None, None, None) == 0
    assert lib.bppp_rp_open_batch(h, 0, None, None, None, None, None, C.byref(acc), None, None) == 0 and acc.value == 1
    assert lib.bppp_rp_open_batch_device(h, 0, 5, None, None, None, None, None, C.byref(acc), None, None) == 0 and acc.value == 1
    assert nat.commit_batch([]) == [] and nat.open_each([], []) == [] and nat.open_batch([], []) is True
    # NULL buffers with a non-empty batch
    assert lib.bppp_rp_commit_batch(h, 2, vp(amt), None, vp(bld), None, vp(cf)) == ERR_ARG
    assert lib.bppp_rp_commit_batch(h, 2, vp(amt), vp(typ), vp(bld), None, None) == ERR_ARG
    assert lib.bppp_rp_commit_batch_device(h, 2, None, None, None, None, None) == ERR_ARG
    assert lib.bppp_rp_open_each(h, 2, vp(cf), vp(amt), vp(typ), vp(bld), None) == ERR_ARG
    assert lib.bppp_rp_open_each(h, 2, None, vp(amt), vp(typ), vp(bld), vp(status)) == ERR_ARG
    assert lib.bppp_rp_open_each_device(h, 2, None, None, None, None, vp(status)) == ERR_ARG
    assert lib.bppp_rp_open_batch(h, 2, vp(cf), vp(amt), vp(typ), vp(bld), None, C.byref(acc), None, None) == ERR_ARG
    assert lib.bppp_rp_open_batch(h, 2, vp(cf), vp(amt), vp(typ), vp(bld), vp(sd), None, None, None) == ERR_ARG
    assert lib.bppp_rp_open_batch_device(h, 2, 0, None, None, None, None, vp(sd), C.byref(acc), None, None) == ERR_ARG
    assert b"null input" in lib.bppp_last_error(gpu.h)
    # batch * nranges >= 2^31 (3 ranges): refused before any buffer is touched
    huge = (2**31 + 2) // 3
    assert lib.bppp_rp_commit_batch(h, huge, vp(amt), vp(typ), vp(bld), None, vp(cf)) == ERR_ARG
    assert lib.bppp_rp_open_each(h, huge, vp(cf), vp(amt), vp(typ), vp(bld), vp(status)) == ERR_ARG
    assert lib.bppp_rp_open_batch(h, huge, vp(cf), vp(amt), vp(typ), vp(bld), vp(sd), C.byref(acc), None, None) == ERR_ARG and acc.value == 0
    assert b"2^31" in lib.bppp_last_error(gpu.h)
    # a binary handle takes NULL types
    bst, binputs, _, _, bwant = _case(oracle_lib, "bin_test")
    bnat = handles("bin_test")
    bamt, _, bbld = bnat._claim_arrays(binputs[:2])
    bcf = np.zeros(2 * bnat.shape["coms_bytes"], dtype=np.uint8)
    assert lib.bppp_rp_commit_batch(bnat.h, 2, vp(bamt), None, vp(bbld), None, vp(bcf)) == 0 and bcf.tobytes() == b"".join(bwant[:2])
    assert lib.bppp_rp_open_each(bnat.h, 2, vp(bcf), vp(bamt), None, vp(bbld), vp(status)) == 0 and not status.any()


def test_closed_context_is_an_argument_error(oracle_lib):
    import bulletproofspp_amd as b_
    st, inputs, _, _, want = _case(oracle_lib, "32bit")
    ctx = b_.Bppp(0)
    nat = _native(ctx, st)
    amt, typ, bld = nat._claim_arrays(inputs[:1])
    cf, status, acc, sd = np.frombuffer(want[0], dtype=np.uint8).copy(), np.zeros(4, dtype=np.uint32), C.c_int(-1), np.frombuffer(SEED, dtype=np.uint8)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    h = nat.h
    ctx.lib.bppp_ctx_destroy(ctx.h)                # the context is closed; the child handle keeps it alive
    ctx.h = None
    try:
        assert ctx.lib.bppp_rp_commit_batch(h, 1, vp(amt), vp(typ), vp(bld), None, vp(cf)) == ERR_ARG
        assert ctx.lib.bppp_rp_open_each(h, 1, vp(cf), vp(amt), vp(typ), vp(bld), vp(status)) == ERR_ARG
        assert ctx.lib.bppp_rp_open_batch(h, 1, vp(cf), vp(amt), vp(typ), vp(bld), vp(sd), C.byref(acc), None, None) == ERR_ARG
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 7. the table is built lazily from either side: the prover's bytes stay
@pytest.mark.parametrize("name", ["rec_test", "bin_test", "64by64"])
def test_prover_bytes_whichever_side_builds_the_table(gpu, oracle_lib, name):
    st, inputs, _, _, want = _case(oracle_lib, name)
    B = 3
    prefixes = [b"table order rnd %04d" % b for b in range(B)]
    first, second = _native(gpu, st), _native(gpu, st)
    try:
        assert first.commit_batch(inputs[:B]) == want[:B]
        proved_after = first.prove_batch(inputs[:B], prefixes)
        proved_before = second.prove_batch(inputs[:B], prefixes)
        assert second.commit_batch(inputs[:B]) == want[:B]
        assert proved_after == proved_before and [c for c, _ in proved_after] == want[:B]
        assert first.verify_batch([c for c, _ in proved_after], [p for _, p in proved_after], SEED)
        # with the prover's comb table in place the commitments go through it instead of the window table: the same files
        first.set_option("comb_bits", 6)
        first.set_option("comb_min", 1)
        assert first.prove_batch(inputs[:B], prefixes) == proved_after and first.comb_info()["points"] > 0
        assert first.commit_batch(inputs[:B]) == want[:B] and first.open_each(want[:B], inputs[:B]) == [[0] * len(st.rds)] * B
        assert first.open_batch(want[:B], inputs[:B], SEED) is True
    finally:
        first.close()
        second.close()
