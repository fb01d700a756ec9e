"""Where the device entry points write.  Every case runs a `_device` entry point of include/bppp.h with EVERY device buffer, inputs and outputs,
sub-allocated from one GuardArena (tests/guard_arena.py): each buffer exactly as long as the header sizes it, at an address = 16 (mod 256) - the
16-byte alignment the header promises and nothing stronger - with guard bytes before, between and behind.  Each case asserts
  (a) the results equal the reference the suite already has for that call: the oracle (oracle/pyoracle.py), or the host protocol code over it, taken
      from the modules that compute them - never the library on another route - and
  (b) arena.check(): no guard byte changed, and no buffer the header declares `const` changed.

CASES below is the completeness table: entry point -> the test here that runs it inside an arena.  tests/test_device_abi_guard_list.py holds it
against include/bppp.h, and every test ends with covered(), which asserts that the entry points the table gives it were really called through the
arena's context (ArenaGpu.lib records every symbol when it is called).

Shapes.  Counts are 1, 3 and 65 (one lane past a wavefront) unless a family says otherwise.  Output buffers whose total length is NOT a multiple of
16 at one count at least: commitment files (33 bytes on `64bit`, 97 on rec_test / bin_test), proof files (418, 546, 578 bytes), 33-byte keys,
65-byte signatures, 66-byte public nonces (odd counts), the `33 n + 32`-byte half-aggregate, seals (226 bytes), glv sign words (4 bytes a scalar),
the new entries of cut-through (4 bytes) and its new pool.  Records of 32 bytes (scalars, partial responses, claims, blindings, openings) and of
64 bytes (points) have no such length: their buffers are checked at their exact length all the same."""
import contextlib
import ctypes as C
import functools
import hashlib
import json
import os
import random
import types

import numpy as np
import pytest

import cut_through_jobs as CJ
import pyoracle as O
import test_gpu_commit_open as CO
import test_gpu_cut_through as CT
import test_gpu_excess as EX
import test_gpu_excess_keys as EK
import test_gpu_poisoned_workspace as PW
import test_gpu_prove_device as PD
import test_gpu_scan_keys as SK
import test_gpu_seal_scan as SS
import test_gpu_tally as TA
from bulletproofspp_amd import capi
from bulletproofspp_amd import encoding as E
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import array_to_point, array_to_scalars, points_to_array, scalars_to_array
from guard_arena import GuardArena, GuardError
from rp_backends import OracleBackend
from test_few_rounds_host import with_public
from test_gpu_decode_conformance import Layout, Lift
from test_gpu_few_rounds import _pool as arg_pool
from test_gpu_few_rounds import run_batch
from test_gpu_seed_points import TP, _lift, _stream
from test_gpu_verify_each import SEED
from test_rangeproof import CASES as RP_CASES
from test_rangeproof import EXAMPLES

pytestmark = pytest.mark.gpu

N, P = O.N, O.P
OK, MALFORMED = 0, 2
VALID, INVALID = 0, 1
COUNTS = (1, 3, 65)

# entry point -> the test below that runs it with every device buffer inside a GuardArena.  Where an output's record is 32 bytes (scalars, claims,
# blindings, openings, partial responses) or 64 bytes (points) no count gives a length that is not a multiple of 16: fold, round, inverse, tensor,
# lift, seed, trrp, tally_claims, part_sign and the scans' openings are checked at their exact length and cannot be checked at an odd one.  Every
# status array of this ABI is host memory; the 4-byte records in HBM are the glv sign words and the new entries of cut-through.
# Counts are 1, 3 and 65 in every family but two: the MSMs (301 and 20011 terms) and the blocks, which run at 1, 4 and 65 proofs with three sums and three
# keys each - the block builder of the poisoned-workspace tests makes every sum gather a proven and an unproven row, so a block has two rows at least.
CASES = {
    "bppp_upload": "test_arena_memory_calls",
    "bppp_download": "test_arena_memory_calls",
    "bppp_fold_points_device": "test_fold_points",
    "bppp_fold_points_eis_device": "test_fold_points",
    "bppp_norm_round_sums_device": "test_round_scalars",
    "bppp_lin_round_sums_device": "test_round_scalars",
    "bppp_norm_round_openings_device": "test_round_scalars",
    "bppp_lin_round_openings_device": "test_round_scalars",
    "bppp_fold_scalars_device": "test_round_scalars",
    "bppp_batch_inverse_device": "test_batch_inverse",
    "bppp_tensor_device": "test_tensor",
    "bppp_glv_decompose_device": "test_glv_decompose",
    "bppp_lift_x_device": "test_lift_x_and_seed_points",
    "bppp_points_from_seed_device": "test_lift_x_and_seed_points",
    "bppp_trrp_public_device": "test_trrp_public",
    "bppp_nl_verify_batch_device": "test_argument_verifiers",
    "bppp_ip_verify_batch_device": "test_argument_verifiers",
    "bppp_msm_device": "test_msm_inputs",
    "bppp_msm_batch_device": "test_msm_inputs",
    "bppp_msm_glv_device": "test_msm_inputs",
    "bppp_msm_basis": "test_msm_inputs",
    "bppp_rp_prove_batch_device": "test_provers",
    "bppp_rp_prove_batch_status_device": "test_provers",
    "bppp_rp_prove_bound_device": "test_provers",
    "bppp_rp_commit_batch_device": "test_balance_calls",
    "bppp_rp_open_each_device": "test_balance_calls",
    "bppp_rp_open_batch_device": "test_balance_calls",
    "bppp_rp_tally_each_device": "test_balance_calls",
    "bppp_rp_tally_batch_device": "test_balance_calls",
    "bppp_rp_tally_claims_device": "test_balance_calls",
    "bppp_rp_excess_sign_device": "test_balance_calls",
    "bppp_rp_excess_verify_each_device": "test_balance_calls",
    "bppp_rp_excess_verify_batch_device": "test_balance_calls",
    "bppp_rp_excess_keys_device": "test_balance_calls",
    "bppp_rp_excess_verify_keys_each_device": "test_balance_calls",
    "bppp_rp_excess_verify_keys_batch_device": "test_balance_calls",
    "bppp_rp_excess_sums_each_device": "test_balance_calls",
    "bppp_rp_excess_sums_batch_device": "test_balance_calls",
    "bppp_rp_excess_part_nonces_device": "test_balance_calls",
    "bppp_rp_excess_part_aggregate_device": "test_balance_calls",
    "bppp_rp_excess_part_sign_device": "test_balance_calls",
    "bppp_rp_excess_part_verify_device": "test_balance_calls",
    "bppp_rp_excess_part_combine_device": "test_balance_calls",
    "bppp_rp_excess_halfagg_device": "test_half_aggregate",
    "bppp_rp_excess_halfagg_verify_device": "test_half_aggregate",
    "bppp_rp_verify_batch_device": "test_verifiers",
    "bppp_rp_verify_each_device": "test_verifiers",
    "bppp_rp_verify_batch_pub_device": "test_verifiers",
    "bppp_rp_verify_each_pub_device": "test_verifiers",
    "bppp_rp_verify_mixed_device": "test_verifiers",
    "bppp_rp_verify_bound_device": "test_verifiers_bound_and_public",
    "bppp_rp_verify_each_bound_device": "test_verifiers_bound_and_public",
    "bppp_rp_verify_block_device": "test_blocks",
    "bppp_rp_verify_block_agg_device": "test_blocks",
    "bppp_rp_seal_device": "test_seal_and_scan",
    "bppp_rp_scan_device": "test_seal_and_scan",
    "bppp_rp_scan_keys_device": "test_scan_keys",
    "bppp_rp_cut_through_device": "test_cut_through",
}


# ----------------------------------------------------------------------------- the harness
class _Recorder:
    """the library, noting every symbol when it is called"""

    def __init__(self, lib, seen):
        self._lib, self._seen = lib, seen

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self._seen.add(name)
            return fn(*args)
        return call


class ArenaGpu(GuardArena):
    """A GuardArena that stands in for the context: alloc, to_device, upload, download and free are the arena's, every other method of capi.Bppp runs
    with the arena as `self` - so what it allocates comes from the arena and what it calls is recorded - and the rest is the context's own."""

    def __init__(self, gpu, capacity_bytes):
        self.called = set()
        self._rec = _Recorder(gpu.lib, self.called)
        super().__init__(gpu, capacity_bytes)

    @property
    def lib(self):
        return self._rec

    def __getattr__(self, name):
        fn = capi.Bppp.__dict__.get(name)
        if isinstance(fn, types.FunctionType):
            return types.MethodType(fn, self)
        return getattr(self.__dict__["gpu"], name)

    def rows(self, ptr, n, width):
        raw = self.download(ptr, (n * width,), np.uint8).tobytes()
        return [raw[t * width:(t + 1) * width] for t in range(n)]

    def last(self, k=1):
        """the pointers of the k buffers handed out last"""
        return [p for p, _ in self.buffer_ranges()[-k:]]


@contextlib.contextmanager
def routed(A, *handles):
    """the handles' wrappers allocate from the arena and call through its recording library while this is open"""
    old = [h.gpu for h in handles]
    for h in handles:
        h.gpu = A
    try:
        yield A
    finally:
        for h, g in zip(handles, old):
            h.gpu = g


@pytest.fixture
def arena(gpu):
    made = []

    def make(capacity=4 << 20):
        made.append(ArenaGpu(gpu, capacity))
        return made[-1]
    yield make
    for a in made:
        a.close()


def covered(called, test):
    """the entry points CASES gives `test` were called through the arena (or arenas: `called` is an ArenaGpu or a set of symbols)"""
    called = getattr(called, "called", called)
    want = {f for f, t in CASES.items() if t == test}
    assert want and want <= called, sorted(want - called)


def _bytes(rows):
    return np.frombuffer(b"".join(rows), dtype=np.uint8)


@pytest.fixture(scope="module")
def nats(gpu, oracle_lib):
    """native handles by (setup key, options), made once"""
    made = {}

    def get(key, **options):
        k = (key, tuple(sorted(options.items())))
        if k not in made:
            made[k] = PW._native(gpu, oracle_lib, key, **options)
        return made[k]
    yield get
    for nat in made.values():
        nat.close()


# ----------------------------------------------------------------------------- 0. the arena's own two calls
def test_arena_memory_calls(arena):
    A = arena(1 << 18)
    rnd = random.Random("guarded memory")
    for n in (1, 33, 418, 4 * 65):
        data = np.frombuffer(bytes(rnd.randrange(256) for _ in range(n)), dtype=np.uint8)
        p = A.alloc(n)
        A.gpu._check(A.lib.bppp_upload(A.h, C.c_void_p(p), C.c_void_p(data.ctypes.data), n), "bppp_upload")
        A.check(outputs=[p])
        back = np.zeros(n, dtype=np.uint8)
        A.gpu._check(A.lib.bppp_download(A.h, C.c_void_p(back.ctypes.data), C.c_void_p(p), n), "bppp_download")
        assert back.tobytes() == data.tobytes()
        assert A.to_device(data) % 256 == 16 and p % 256 == 16
    A.check()
    # the check sees the card's memory, not a copy: one byte behind a buffer, then one byte of an input, written inside the arena's own allocation
    (p33, _), (q33, _) = A.buffer_ranges()[2:4]                    # the 33-byte output and the 33-byte input uploaded after it
    for addr, side, at in ((p33 + 33, "after", 33), (q33 + 7, "input", 7)):
        old = A.gpu.download(addr, (1,), np.uint8)
        A.gpu.upload(addr, old ^ np.uint8(0xFF))
        with pytest.raises(GuardError) as e:
            A.check()
        assert (e.value.side, e.value.first, e.value.last, e.value.count) == (side, at, at, 1) and "[33 bytes]" in str(e.value)
        A.gpu.upload(addr, old)
    A.check()
    covered(A, "test_arena_memory_calls")


# ----------------------------------------------------------------------------- 1. context vector calls
@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_fold_points(arena, oracle_lib, n):
    """out is ceil(n / 2) points of 64 bytes: an odd n pairs its tail with infinity and must not write the slot behind"""
    A, ec = arena(1 << 18), oracle_lib
    rnd = random.Random("guarded fold %d" % n)
    pts = O.hash_points(b"guarded fold %d" % n, n)
    if n > 4:
        pts[3] = None
    e, half = rnd.randrange(N), (n + 1) // 2
    right = lambda j: pts[2 * j + 1] if 2 * j + 1 < n else None
    a1, b1 = O.rational_reduce_scalar(e)
    d_p, d_o = A.to_device(points_to_array(pts)), A.alloc(half * 64)
    A.fold_points_device(b1, a1, d_p, n, d_o)
    assert [array_to_point(r) for r in A.download(d_o, (half, 8))] == [ec.pair_ip(b1, pts[2 * j], a1, right(j)) for j in range(half)]
    A.check(outputs=[d_o])
    a2, b2 = O.rational_reduce_scalar_eis(e)
    out = A.fold_points_eis(b2, a2, points_to_array(pts))          # uploads the points again and takes ceil(n / 2) * 64 bytes for the output
    assert [array_to_point(r) for r in out] == [O.pair_ip_eis(b2, pts[2 * j], a2, right(j), ec) for j in range(half)]
    assert A.buffer_ranges()[-1][1] == half * 64
    A.check(outputs=A.last())
    covered(A, "test_fold_points")


@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_round_scalars(arena, n):
    A = arena(1 << 18)
    rnd = random.Random("guarded rounds %d" % n)
    x, c = [rnd.randrange(N) for _ in range(n)], [rnd.randrange(N) for _ in range(n)]
    q = rnd.randrange(1, N)
    qi, npair = O.inv_mod(q, N), (n + 1) // 2
    dx, dc = A.to_device(scalars_to_array(x)), A.to_device(scalars_to_array(c))
    # Norm.makeScalarsComs (NormArgument.hs:113-118)
    sX, xw, sR, rw = O.Norm(q, qi, 1, [(v, None) for v in x]).make_scalars_coms()
    q4 = pow(q, 4, N)
    sx, sr = A.norm_round_sums(dx, n, q4)
    assert 2 * pow(q, 3, N) * sx % N == sX and q4 * sr % N == sR
    dxw, drw = A.alloc(2 * npair * 32), A.alloc(npair * 32)
    A.norm_round_openings(dx, n, q, qi, dxw, drw)
    assert array_to_scalars(A.download(dxw, (2 * npair, 4))) == [v for v, _ in xw.body]
    assert array_to_scalars(A.download(drw, (npair, 4))) == [v for v, _ in rw.body]
    A.check(outputs=[dxw, drw])
    # Linear.makeScalarsComs (NormArgument.hs:56-59)
    lX, lxw, lR, lrw = O.Linear(1, [(cc, v, None) for cc, v in zip(c, x)]).make_scalars_coms()
    assert A.lin_round_sums(dc, dx, n) == (lX, lR)
    dxw, drw = A.alloc(2 * npair * 32), A.alloc(npair * 32)
    A.lin_round_openings(dx, n, dxw, drw)
    assert array_to_scalars(A.download(dxw, (2 * npair, 4))) == [v for _, v, _ in lxw.body]
    assert array_to_scalars(A.download(drw, (npair, 4))) == [v for _, v, _ in lrw.body]
    A.check(outputs=[dxw, drw])
    u, v = rnd.randrange(N), rnd.randrange(N)
    dout = A.alloc(npair * 32)
    A.fold_scalars(u, v, dx, n, dout)
    assert array_to_scalars(A.download(dout, (npair, 4))) == [(u * x[2 * j] + (v * x[2 * j + 1] if 2 * j + 1 < n else 0)) % N for j in range(npair)]
    A.check(outputs=[dout])
    covered(A, "test_round_scalars")


@pytest.mark.parametrize("n", [1, 7, 8, 9, 513])                   # around BI_RUN = 8 values a lane, and one value past 64 full lanes
@pytest.mark.parametrize("mod,m", [(0, P), (1, N)])
def test_batch_inverse(arena, mod, m, n):
    A = arena(1 << 18)
    rnd = random.Random("guarded inverse %d %d" % (mod, n))
    xs = [rnd.randrange(m) for _ in range(n)]
    for i in range(0, n, 5):
        xs[i] = 0
    if n > 3:
        xs[3] = m - 1
    want = O.batch_inverse(xs, m)
    dx, dout = A.to_device(scalars_to_array(xs)), A.alloc(n * 32)
    A.batch_inverse(dx, n, mod, dout)                              # out of place: the input stays
    assert array_to_scalars(A.download(dout, (n, 4))) == want
    A.check(outputs=[dout])
    A.batch_inverse(dx, n, mod, dx)                                # in place
    assert array_to_scalars(A.download(dx, (n, 4))) == want
    A.check(outputs=[dx])
    covered(A, "test_batch_inverse")


@pytest.mark.parametrize("nb,k", [(1, 0), (3, 1), (1, 6), (65, 1)])
def test_tensor(arena, nb, k):
    A = arena(1 << 18)
    rnd = random.Random("guarded tensor %d %d" % (nb, k))
    bs, es, qs = ([rnd.randrange(N) for _ in range(c)] for c in (nb, k, k))
    dout = A.alloc((nb << k) * 32)
    A.tensor(bs, es, qs, dout)
    assert array_to_scalars(A.download(dout, (nb << k, 4))) == O.tensor(bs, es, lambda r: qs[r])
    A.check(outputs=[dout])
    covered(A, "test_tensor")


@pytest.mark.parametrize("n", COUNTS)
def test_glv_decompose(arena, n):
    """three outputs; d_signs is [n] uint32: 4, 12 and 260 bytes here, none a multiple of 16"""
    A = arena(1 << 18)
    rnd = random.Random("guarded glv %d" % n)
    xs = ([N - 1, O.LAMBDA, 2**255 + 12345] + [rnd.randrange(N) for _ in range(n)])[:n]
    d_s, d_a, d_b, d_g = A.to_device(scalars_to_array(xs)), A.alloc(n * 32), A.alloc(n * 32), A.alloc(n * 4)
    p = C.c_void_p
    A.gpu._check(A.lib.bppp_glv_decompose_device(A.h, p(d_s), n, p(d_a), p(d_b), p(d_g)), "bppp_glv_decompose_device")
    a, b = array_to_scalars(A.download(d_a, (n, 4))), array_to_scalars(A.download(d_b, (n, 4)))
    f = [int(v) for v in A.download(d_g, (n,), np.uint32)]
    assert [(-x if s & 1 else x, -y if s & 2 else y) for x, y, s in zip(a, b, f)] == [O.decompose_eis(x) for x in xs] and not any(s & ~3 for s in f)
    A.check(outputs=[d_a, d_b, d_g])
    covered(A, "test_glv_decompose")


@pytest.mark.parametrize("n", COUNTS)
def test_lift_x_and_seed_points(arena, n):
    A = arena(1 << 18)
    rnd = random.Random("guarded lift %d" % n)
    xs = [rnd.randrange(P) for _ in range(n)]
    if n > 2:
        xs[1], xs[2] = P + 5, next(x for x in range(2, 200) if _lift(x) is None)
    d_x, d_p = A.to_device(scalars_to_array(xs)), A.alloc(n * 64)
    A.lift_x(d_x, n, d_p)
    assert [array_to_point(r) for r in A.download(d_p, (n, 8))] == [None if x >= P else _lift(x) for x in xs]
    A.check(outputs=[d_p])
    want = _stream(TP, n)
    d_pts, nxt = A.points_from_seed(TP, n, device=True)            # takes count * 64 bytes from the arena
    assert A.buffer_ranges()[-1] == (d_pts, n * 64)
    assert [array_to_point(r) for r in A.download(d_pts, (n, 8))] == [pt for _, pt in want] and nxt == want[-1][0] + 1
    A.check(outputs=[d_pts])
    covered(A, "test_lift_x_and_seed_points")


@functools.lru_cache(maxsize=None)
def _trrp_reference(name, flavour):
    """(setup over the oracle, 65 challenge rows, the host derivation of each: q, sp, pub_norm, pub_lin_c, init scalars)"""
    ec = O.CEC()
    ranges, typed, pub, vals = RP_CASES[name]
    st = RP.setup(OracleBackend(ec), O.hash_points(b"test points", 300), typed, pub, [RP.make_range_data(*r) for r in ranges], flavour)
    rnd = random.Random("guarded trrp " + name)
    proof = RP.prove(st, RP.witness(st, [(v, ty, rnd.randrange(N)) for v, ty in vals]), RP.sha256_oracle(), RP.hash_to_scalar(b"g"))
    chs = [[1, 2, 3, 4, 5, 6, 7], [N - 1] * 7] + [[rnd.randrange(N) for _ in range(7)] for _ in range(63)]
    pad = lambda xs, n: list(xs) + [0] * (n - len(xs))
    want = []
    for e, x, r0, q, xp, r1, t in chs:
        seq = iter([[e, x, r0], [q, xp, r1], [t]])
        sbp = RP.verify_rp(st, proof.coms, RP.Transcript(lambda cs, n: next(seq)))
        by_point = {}
        for s_, p_ in sbp.init_terms:
            by_point[p_] = (by_point.get(p_, 0) + s_) % N
        want.append(([q % N], [sbp.pub.sc], pad(sbp.pub.nrm, st.nrm_len), pad(sbp.cs, st.lin_len), [by_point[p_] for p_ in proof.coms]))
    return st, chs, want


@pytest.mark.parametrize("batch", [1, 65, 1025])                   # 1025: the three-kernel route (above 1024 proofs)
def test_trrp_public(arena, gpu, batch):
    """five output arrays of 32-byte scalars; row b of a batch is challenge row b mod 65, so every row has its host derivation"""
    st, chs, want = _trrp_reference("typed_with_assumed", "NL")
    A = arena(8 << 20)
    tabs = RP.DeviceVerifierTables(gpu, st)
    try:
        per = [1, 1, st.nrm_len, st.lin_len, tabs.ninit]
        d_ch = A.to_device(np.concatenate([scalars_to_array(chs[b % 65]) for b in range(batch)]))
        outs = [A.alloc(batch * k * 32) for k in per]
        with routed(A, tabs):
            tabs.public_device(batch, d_ch, *outs)
        for i, (d, k) in enumerate(zip(outs, per)):
            got = array_to_scalars(A.download(d, (batch * k, 4)))
            assert got == [v for b in range(batch) for v in want[b % 65][i]], i
        A.check(outputs=outs)
    finally:
        tabs.close()
    covered(A, "test_trrp_public")


@pytest.mark.parametrize("batch", COUNTS)
def test_argument_verifiers(arena, oracle_lib, batch):
    """the smallest shape of test_gpu_few_rounds.py, no round at all: fifteen input arrays each, one of them a single scalar"""
    A = arena(1 << 20)
    for key in (("NL", 1, 1), ("IP", 1, 1)):
        pool = arg_pool(oracle_lib, key, 0)
        arrs, want = PW._arg_batch(oracle_lib, pool, batch, 3)
        assert run_batch(A, pool, batch, arrs) == (0, want)
        A.check(outputs=[])
    covered(A, "test_argument_verifiers")


@pytest.mark.parametrize("n,c", [(301, 0), (301, 13), (20011, 13), (20011, 16)])
def test_msm_inputs(arena, oracle_lib, n, c):
    """the MSMs write no caller buffer in HBM: scalars and points stay as uploaded, whatever the sort and the buckets do around them"""
    A, ec = arena(16 << 20), oracle_lib
    rows, idx, want = PW._msm_case(ec, "msm", c, n, 1, "dense", 31)
    assert PW._msm_call(A, "msm", c, n, 1, rows, idx)() == want
    ds, dp = A.last(2)
    assert A.msm_glv_device(ds, dp, n) == want[0]
    A.check(outputs=[])
    if n == 301:
        for kind, cb in (("batch shared", 5), ("batch own", 8), ("basis", 8)):
            rows, idx, want = PW._msm_case(ec, kind, cb, n, 3, "edge", 32)
            basis = A.basis(np.ascontiguousarray(PW._msm_base()[1][np.arange(n) % PW.NBASE]), window_bits=cb, batch_hint=3) if kind == "basis" else None
            try:
                assert PW._msm_call(A, kind, cb, n, 3, rows, idx, basis)() == want
            finally:
                if basis is not None:
                    basis.close()
            A.check(outputs=[])
        covered(A, "test_msm_inputs")
    else:                                                           # two instances over one basis and over a basis each, at this window width
        for kind in ("batch shared", "batch own"):
            rows, idx, want = PW._msm_case(ec, kind, c, n, 2, "dense", 33)
            assert PW._msm_call(A, kind, c, n, 2, rows, idx)() == want
            A.check(outputs=[])
        assert {"bppp_msm_device", "bppp_msm_glv_device", "bppp_msm_batch_device"} <= A.called


# ----------------------------------------------------------------------------- 2. the provers
PROVE_JS = (50, 51, 52)                                            # three host proofs a setup; proof b of a batch is number b mod 3
COMB = dict(PW.COMB, host_oracle_max=0)                            # a small comb table and the device oracle: the stream of kernels that ends in the encoder
# The refused proof has its first amount raised above its range.  include/bppp.h: a typed handle reports the lowest code that applies, and on rec_test
# (1 + in1 + in2 = out) the raised amount breaks the balance first; 64bit has nothing to balance; a binary handle reports the first offending range.
REFUSAL = {"64bit": capi.RP_WIT_OUT_OF_RANGE, "rec_test": capi.RP_WIT_UNBALANCED, "bin_test": capi.RP_WIT_OUT_OF_RANGE}


@pytest.mark.parametrize("name", ["64bit", "rec_test", "bin_test"])
def test_provers(arena, gpu, oracle_lib, nats, name):
    """tail buffers: the commitment files (33 bytes a proof on 64bit, 97 on the other two) and the proof files (418, 546, 578 bytes), at 1, 3 and 65
    proofs; a refused proof's files are zeroed inside their rows"""
    key, ec = (name, None), oracle_lib
    nat = nats(key, **COMB)
    A = arena(2 << 20)
    st = PW._host_setup(ec, key)[0]
    cb, pb = nat.shape["coms_bytes"], nat.shape["proof_bytes"]
    assert (cb % 16, pb % 16) != (0, 0)
    for B in COUNTS:
        js = [PROVE_JS[b % 3] for b in range(B)]
        inputs, prefixes = [PW._rows(ec, key, j) for j in js], [PW._prefix(j) for j in js]
        want = PW.host_files(key, js)
        with routed(A, nat):
            # bppp_rp_prove_batch_device
            with PD._DeviceCall(nat, inputs, prefixes, alloc=A) as dc:
                assert A.buffer_ranges()[-2:] == [(dc.d["cf"], B * cb), (dc.d["pf"], B * pb)]
                assert dc.device_files() == want, B
                A.check(outputs=[dc.d["cf"], dc.d["pf"]])
            # bppp_rp_prove_batch_status_device, proof B // 2 refused: its first amount lies above its range
            bad = B // 2
            rows = [list(r) for r in inputs]
            rows[bad][0] = (st.rds[0].hi + 3,) + tuple(rows[bad][0][1:])
            zero = (bytes(cb), bytes(pb))
            with PD._DeviceCall(nat, rows, prefixes, alloc=A) as dc:
                d = dc.d
                status = nat.prove_batch_status_device(B, d["amt"], 0 if dc.binary else d["typ"], d["bld"], d["pre"], dc.plen, d["cf"], d["pf"])
                assert [int(s) for s in status] == [REFUSAL[name] if b == bad else capi.RP_WIT_OK for b in range(B)]
                got = nat._prove_files(B, A.download(d["cf"], dc.cf.shape, np.uint8), A.download(d["pf"], dc.pf.shape, np.uint8))
                assert got == [zero if b == bad else f for b, f in enumerate(want)], B
                A.check(outputs=[d["cf"], d["pf"]])
            # bppp_rp_prove_bound_device, the bindings in HBM too
            bind = {j: hashlib.sha256(b"guarded binding %d" % j).digest() for j in PROVE_JS}
            bound = PW.host_files(key, PROVE_JS, bindings=tuple(bind[j] for j in PROVE_JS))
            with PD._DeviceCall(nat, inputs, prefixes, alloc=A) as dc:
                d = dc.d
                d_bind = A.to_device(_bytes([bind[j] for j in js]))
                nat.prove_batch_device(B, d["amt"], 0 if dc.binary else d["typ"], d["bld"], d["pre"], dc.plen, d["cf"], d["pf"], bindings=d_bind)
                got = nat._prove_files(B, A.download(d["cf"], dc.cf.shape, np.uint8), A.download(d["pf"], dc.pf.shape, np.uint8))
                assert got == [bound[b % 3] for b in range(B)], B
                A.check(outputs=[d["cf"], d["pf"]])
    # the slow path of the device entry point: a handle without a comb table downloads the inputs, proves through host buffers and uploads the files
    slow = nats(key)
    assert slow.comb_info()["points"] == 0
    js = list(PROVE_JS)
    with routed(A, slow), PD._DeviceCall(slow, [PW._rows(ec, key, j) for j in js], [PW._prefix(j) for j in js], alloc=A) as dc:
        assert dc.device_files() == PW.host_files(key, js)
        A.check(outputs=[dc.d["cf"], dc.d["pf"]])
    assert slow.comb_info()["points"] == 0
    covered(A, "test_provers")


# ----------------------------------------------------------------------------- 3. commit, open, tally and the excess signatures
class Twin:
    """The host wrappers' signatures over the _device entry points: every array goes into the arena at its exact length, the call runs, the outputs
    come back in the host wrapper's shape, and the arena is checked with exactly the call's outputs named.  A job of test_gpu_poisoned_workspace.Balance
    - whose expected values are the host protocol code's - therefore runs on a Twin as it runs on a handle."""

    def __init__(self, nat, A):
        self.nat, self.A, self.binary = nat, A, isinstance(nat, BRP.NativeBinaryRangeProofs)

    def _up(self, *arrays):
        return [self.A.to_device(a if isinstance(a, np.ndarray) else _bytes(a)) for a in arrays]

    # ---- commit and open
    def commit_batch(self, inputs):
        A, nat = self.A, self.nat
        with routed(A, nat), CO._Dev(nat, inputs, alloc=A) as dev:
            assert A.buffer_ranges()[-1] == (dev.d["cf"], len(inputs) * nat.shape["coms_bytes"])
            status = nat.commit_batch_device(dev.B, *dev.claims(), dev.d["cf"], want_status=True)
            assert list(status) == [0] * dev.B
            files = dev.files()
        A.check(outputs=[dev.d["cf"]])
        return files

    def open_each(self, files, inputs):
        A, nat = self.A, self.nat
        with routed(A, nat), CO._Dev(nat, inputs, files, alloc=A) as dev:
            out = nat.open_each_device(dev.B, dev.d["cf"], *dev.claims())
        A.check(outputs=[])
        return out

    def open_batch(self, files, inputs, seed, want_status=False, want_point=False):
        A, nat = self.A, self.nat
        with routed(A, nat), CO._Dev(nat, inputs, files, alloc=A) as dev:
            out = nat.open_batch_device(dev.B, dev.d["cf"], *dev.claims(), seed=seed, want_status=want_status, want_point=want_point)
        A.check(outputs=[])
        return out

    # ---- tallies
    def tally_each(self, files, ss, en, claims=None, want_points=False):
        A, nat = self.A, self.nat
        with routed(A, nat), TA._Dev(nat, files, ss, en, claims, alloc=A) as dev:
            out = nat.tally_each_device(*dev.args(), want_points=want_points)
        A.check(outputs=[])
        return out

    def tally_batch(self, files, ss, en, claims, seed, want_status=False, want_point=False):
        A, nat = self.A, self.nat
        with routed(A, nat), TA._Dev(nat, files, ss, en, claims, alloc=A) as dev:
            out = nat.tally_batch_device(*dev.args(), seed=seed, want_status=want_status, want_point=want_point)
        A.check(outputs=[])
        return out

    def tally_claims(self, inputs, ss, en):
        A, nat = self.A, self.nat
        amt, typ, bld = nat._claim_arrays(inputs)
        ssa, ena, nsums, nnz = nat._tally_csr(ss, en)
        d_amt, d_bld, d_ss, d_en = self._up(amt, bld, ssa, ena)
        d_typ = 0 if self.binary else A.to_device(typ)
        outs = [A.alloc(32 * nsums), 0 if self.binary else A.alloc(32 * nsums), A.alloc(32 * nsums)]
        with routed(A, nat):
            nat.tally_claims_device(len(inputs), d_amt, d_typ, d_bld, nsums, d_ss, d_en, nnz, *outs)
        a, ty, e = ([0] * nsums if not d else array_to_scalars(A.download(d, (nsums, 4))) for d in outs)
        A.check(outputs=outs)
        return nat._tally_claims_shape([((v - 2**256 if v >= 2**255 else v) % N, t, b) for v, t, b in zip(a, ty, e)])

    # ---- excess signatures over the sums
    def excess_sign(self, es, msgs, aux, want_status=False, want_points=False):
        A, nat, n = self.A, self.nat, len(es)
        d_bl, d_mg = self._up(scalars_to_array(es), msgs)
        d_sg = A.alloc(n * RP.EXCESS_SIG_BYTES)
        with routed(A, nat):
            st, pts = nat.excess_sign_device(n, d_bl, d_mg, d_sg, aux, want_status=want_status, want_points=want_points)
        sigs = A.rows(d_sg, n, RP.EXCESS_SIG_BYTES)
        A.check(outputs=[d_sg])
        return sigs, st, pts

    def excess_verify_each(self, files, ss, en, public, msgs, sigs):
        A, nat = self.A, self.nat
        with routed(A, nat), EX._Dev(nat, files, ss, en, public, msgs, sigs, alloc=A) as dev:
            out = nat.excess_verify_each_device(*dev.args())
        A.check(outputs=[])
        return out

    def excess_verify_batch(self, files, ss, en, public, msgs, sigs, seed, want_status=False, want_point=False):
        A, nat = self.A, self.nat
        with routed(A, nat), EX._Dev(nat, files, ss, en, public, msgs, sigs, alloc=A) as dev:
            out = nat.excess_verify_batch_device(*dev.args(), seed=seed, want_status=want_status, want_point=want_point)
        A.check(outputs=[])
        return out

    # ---- stated keys
    def excess_keys(self, es, want_status=False):
        A, nat, n = self.A, self.nat, len(es)
        (d_bl,), d_ks = self._up(scalars_to_array(es)), A.alloc(n * RP.EXCESS_KEY_BYTES)
        with routed(A, nat):
            st = nat.excess_keys_device(n, d_bl, d_ks, want_status=want_status)
        keys = A.rows(d_ks, n, RP.EXCESS_KEY_BYTES)
        A.check(outputs=[d_ks])
        return keys, st

    def excess_verify_keys_each(self, keys, msgs, sigs):
        A, nat = self.A, self.nat
        d = self._up(keys, msgs, sigs)
        with routed(A, nat):
            out = nat.excess_verify_keys_each_device(len(keys), *d)
        A.check(outputs=[])
        return out

    def excess_verify_keys_batch(self, keys, msgs, sigs, seed, want_status=False, want_point=False):
        A, nat = self.A, self.nat
        d = self._up(keys, msgs, sigs)
        with routed(A, nat):
            out = nat.excess_verify_keys_batch_device(len(keys), *d, seed=seed, want_status=want_status, want_point=want_point)
        A.check(outputs=[])
        return out

    def excess_sums_each(self, files, ss, en, claims, key_start, keys, want_points=False):
        A, nat = self.A, self.nat
        dev, args = EK._sums_dev(nat, files, ss, en, claims, key_start, keys, alloc=A)
        with routed(A, nat), dev as d:
            out = nat.excess_sums_each_device(*args(d), want_points=want_points)
        A.check(outputs=[])
        return out

    def excess_sums_batch(self, files, ss, en, claims, key_start, keys, seed, want_status=False, want_point=False):
        A, nat = self.A, self.nat
        dev, args = EK._sums_dev(nat, files, ss, en, claims, key_start, keys, alloc=A)
        with routed(A, nat), dev as d:
            out = nat.excess_sums_batch_device(*args(d), seed=seed, want_status=want_status, want_point=want_point)
        A.check(outputs=[])
        return out

    # ---- the multi-party signer
    def excess_part_nonces(self, blinds, msgs, aux, want_status=False):
        A, nat, n = self.A, self.nat, len(blinds)
        d_bl, d_mg = self._up(scalars_to_array(blinds), msgs)
        d_pn = A.alloc(n * RP.EXCESS_PUBNONCE_BYTES)
        with routed(A, nat):
            st = nat.excess_part_nonces_device(n, d_bl, d_mg, d_pn, aux, want_status=want_status)
        out = A.rows(d_pn, n, RP.EXCESS_PUBNONCE_BYTES)
        A.check(outputs=[d_pn])
        return out, st

    def excess_part_aggregate(self, part_start, pubnonces, keys, want_status=False):
        A, nat, ns, npart = self.A, self.nat, len(part_start) - 1, len(pubnonces)
        d = self._up(np.array(part_start, dtype=np.uint32), pubnonces, keys)
        d_an, d_ak = A.alloc(ns * RP.EXCESS_PUBNONCE_BYTES), A.alloc(ns * RP.EXCESS_KEY_BYTES)
        with routed(A, nat):
            st = nat.excess_part_aggregate_device(ns, npart, *d, d_an, d_ak, want_status=want_status)
        out = A.rows(d_an, ns, RP.EXCESS_PUBNONCE_BYTES), A.rows(d_ak, ns, RP.EXCESS_KEY_BYTES)
        A.check(outputs=[d_an, d_ak])
        return out + (st,)

    def excess_part_sign(self, blinds, msgs, aux, agg_nonces, agg_keys, want_status=False):
        A, nat, n = self.A, self.nat, len(blinds)
        d = self._up(scalars_to_array(blinds), msgs, agg_nonces, agg_keys)
        d_pt = A.alloc(n * RP.EXCESS_PARTIAL_BYTES)
        with routed(A, nat):
            st = nat.excess_part_sign_device(n, *d, d_pt, aux, want_status=want_status)
        out = A.rows(d_pt, n, RP.EXCESS_PARTIAL_BYTES)
        A.check(outputs=[d_pt])
        return out, st

    def excess_part_verify(self, part_start, pubnonces, keys, partials, msgs):
        A, nat = self.A, self.nat
        d = self._up(np.array(part_start, dtype=np.uint32), pubnonces, keys, partials, msgs)
        with routed(A, nat):
            out = nat.excess_part_verify_device(len(part_start) - 1, len(pubnonces), *d)
        A.check(outputs=[])
        return out

    def excess_part_combine(self, part_start, pubnonces, keys, partials, msgs, want_status=False, want_keys=False):
        A, nat, ns = self.A, self.nat, len(part_start) - 1
        d = self._up(np.array(part_start, dtype=np.uint32), pubnonces, keys, partials, msgs)
        d_sg, d_ak = A.alloc(ns * RP.EXCESS_SIG_BYTES), A.alloc(ns * RP.EXCESS_KEY_BYTES)
        with routed(A, nat):
            st = nat.excess_part_combine_device(ns, len(pubnonces), *d, d_sg, d_ak, want_status=want_status)
        out = A.rows(d_sg, ns, RP.EXCESS_SIG_BYTES), A.rows(d_ak, ns, RP.EXCESS_KEY_BYTES)
        A.check(outputs=[d_sg, d_ak])
        return out[0], st, out[1]

    # ---- half-aggregates
    def excess_halfagg(self, keys, msgs, sigs, want_status=False):
        A, nat, n = self.A, self.nat, len(keys)
        d = self._up(keys, msgs, sigs)
        d_agg = A.alloc(RP.EXCESS_AGG_BYTES(n))
        with routed(A, nat):
            st = nat.excess_halfagg_device(n, *d, d_agg, want_status=want_status)
        out = A.download(d_agg, (RP.EXCESS_AGG_BYTES(n),), np.uint8).tobytes()
        A.check(outputs=[d_agg])
        return out, st

    def excess_halfagg_verify(self, keys, msgs, agg, want_status=False, want_point=False):
        A, nat = self.A, self.nat
        d = self._up(keys, msgs, [agg])
        with routed(A, nat):
            out = nat.excess_halfagg_verify_device(len(keys), *d, want_status=want_status, want_point=want_point)
        A.check(outputs=[])
        return out


BAL_NAMES = PW.BAL_NAMES                                           # rec_test (typed) and bin_test (binary): 3 ranges, files of 97 bytes
_JOBS = {}


def _job(ec, name, count):
    """a Balance job of `count` rows and `count` sums (3 or 65): 2 * count parts, one mismatch and one malformed member in every verifying call"""
    if (name, count) not in _JOBS:
        _JOBS[name, count] = PW.Balance(ec, name, list(range(count)), 40 + count, count)
    return _JOBS[name, count]


@pytest.fixture(scope="module")
def balance_handles(gpu, oracle_lib):
    made = {name: CO._native(gpu, CO._case(oracle_lib, name)[0]) for name in BAL_NAMES}
    yield made
    for nat in made.values():
        nat.close()


@pytest.mark.parametrize("name", BAL_NAMES)
def test_balance_calls(arena, oracle_lib, balance_handles, name):
    """every balance call of test_gpu_poisoned_workspace.Balance through its _device entry point, at 3 and 65 rows and sums (files of 97 bytes, keys of
    33, signatures of 65, public nonces of 66: none of the totals a multiple of 16), then every call at a count of one"""
    nat, ec, called = balance_handles[name], oracle_lib, set()
    for count in (3, 65):
        job = _job(ec, name, count)
        assert set(job.calls) == set(PW.BAL_CALLS)
        for what in PW.BAL_CALLS:
            A = arena(2 << 20)
            make, want = job.calls[what]
            assert PW._plain(make(Twin(nat, A))()) == PW._plain(want), (count, what)
            called |= A.called
    # the calls with an output at one row, one sum, one session, one sum of two parts: the first of the job of three
    v, A = _job(ec, name, 3).v, arena(1 << 20)
    tw = Twin(nat, A)
    one = v.sum_start[1]
    assert tw.commit_batch(v.inputs[:1]) == v.files[:1]
    assert PW._plain(tw.tally_claims(v.inputs, v.sum_start[:2], v.entries[:one])) == PW._plain(v.claims[:1])
    assert tw.excess_sign(v.blinds[:1], v.msgs[:1], PW.AUX, want_status=True, want_points=True) == (v.sigs[:1], [OK], v.excess_points[:1])
    assert tw.excess_keys(v.blinds[:1], want_status=True) == (v.keys[:1], [OK])
    assert tw.excess_part_nonces(v.part_blinds[:1], v.part_msgs[:1], PW.AUX, want_status=True) == (v.part_nonces[:1], [OK])
    assert v.part_start[:2] == [0, 2]
    two = (v.part_start[:2], v.part_nonces[:2], v.part_keys[:2])
    assert tw.excess_part_aggregate(*two, want_status=True) == (v.agg_nonces[:1], v.agg_keys[:1], [OK])
    assert tw.excess_part_sign(v.part_blinds[:1], v.part_msgs[:1], PW.AUX, v.agg_nonces[:1], v.agg_keys[:1], want_status=True) == (v.partials[:1], [OK])
    status, sig, key = v.combined[0]
    assert tw.excess_part_combine(*two, v.partials[:2], v.msgs[:1], want_status=True, want_keys=True) == ([sig], [status], [key])
    _verifying_calls_at_one(tw, ec, name, v)
    covered(called | A.called, "test_balance_calls")


def _verifying_calls_at_one(tw, ec, name, v):
    """The calls that only read HBM at ONE row (three commitments), one sum, one key, one signature - a Balance job cannot be that small, for it wants a
    mismatched and a malformed member in every call.  Each call runs once honest and once with its one member wrong; the verdicts and points are the host
    protocol code's over the oracle."""
    st, inputs, triples, pts, files = CO._case(ec, name)
    be, binary, nr = OracleBackend(ec), name == "bin_test", len(st.rds)
    g, _, Bp = RP._excess_bases(st)
    row, trip, file = [inputs[0]], triples[0], [files[0]]
    ss, en = [0, 2], [RP.tally_entry(0, False), RP.tally_entry(nr - 1, True)]
    claim = RP.tally_claims_host(trip, ss, en)[0]
    S = RP.tally_sums(be, pts[0], ss, en)[0]
    cut = (lambda c: (c[0], c[2])) if binary else (lambda c: tuple(c))
    off_by_one = ((claim[0] + 1) % N,) + tuple(claim[1:])
    ok_grid, seed = [[OK] * nr], PW.BAL_SEED
    # openings: the claimed amount of commitment 1 off by one
    wrong_row = [list(row[0])]
    wrong_row[0][1] = (row[0][1][0] + 1,) + tuple(row[0][1][1:])
    bad_grid = [[PW.MISMATCH if i == 1 else OK for i in range(nr)]]
    assert tw.open_each(file, row) == ok_grid and tw.open_each(file, wrong_row) == bad_grid
    assert PW._plain(tw.open_batch(file, row, seed, want_status=True, want_point=True)) == [True, ok_grid, None]
    assert PW._plain(tw.open_batch(file, wrong_row, seed, want_status=True)) == [False, bad_grid, None]
    # the tally of the one sum
    assert PW._plain(tw.tally_each(file, ss, en, [cut(claim)], want_points=True)) == PW._plain([[OK], [S]])
    assert PW._plain(tw.tally_each(file, ss, en, [cut(off_by_one)], want_points=True)) == PW._plain([[PW.MISMATCH], [S]])
    assert PW._plain(tw.tally_batch(file, ss, en, [cut(claim)], seed, want_status=True, want_point=True)) == [True, [OK], None]
    assert PW._plain(tw.tally_batch(file, ss, en, [cut(off_by_one)], seed, want_status=True)) == [False, [PW.MISMATCH], None]
    # the excess signature over it, and the same signature with s + 1
    msg = hashlib.sha256(b"guarded one sum " + name.encode()).digest()
    code, sig, X = RP.excess_sign_host(be, st, claim[2], msg, PW.AUX)
    assert code == 0
    bent = EK._with_s(sig, (EK._s_of(sig) + 1) % N)
    public = [claim[:1] if binary else claim[:2]]
    host_claim = (claim[0],) if binary else claim
    for sg in (sig, bent):
        want = RP.excess_verify_host(be, st, S, host_claim, msg, sg, malformed=False)
        assert want == (OK if sg is sig else PW.MISMATCH)
        assert tw.excess_verify_each(file, ss, en, public, [msg], [sg]) == [want]
        assert PW._plain(tw.excess_verify_batch(file, ss, en, public, [msg], [sg], seed, want_status=True)) == [want == OK, [want], None]
        key = RP.excess_key33(X)
        want_k = RP.excess_verify_key_host(be, st, key, msg, sg)
        assert want_k == want
        assert tw.excess_verify_keys_each([key], [msg], [sg]) == [want_k]
        assert PW._plain(tw.excess_verify_keys_batch([key], [msg], [sg], seed, want_status=True)) == [want_k == OK, [want_k], None]
    # the sum against one stated key: the offset takes the rest of the blinding sum
    x = random.Random("guarded one key " + name).randrange(1, N)
    skey = [RP.excess_key33(be.commit([x], [Bp]))]
    for c3 in ((claim[0], claim[1], (claim[2] - x) % N), (off_by_one[0], claim[1], (claim[2] - x) % N)):
        want, point = RP.excess_sums_host(be, st, S, (c3[0], c3[2]) if binary else c3, skey, malformed=False)
        assert want == (OK if c3[0] == claim[0] else PW.MISMATCH)
        assert PW._plain(tw.excess_sums_each(file, ss, en, [cut(c3)], [0, 1], skey, want_points=True)) == PW._plain([[want], [point]])
        assert PW._plain(tw.excess_sums_batch(file, ss, en, [cut(c3)], [0, 1], skey, seed, want_status=True)) == [want == OK, [want], None]
    # one sum of two parts, honest and with the second partial off by one
    two = (v.part_start[:2], v.part_nonces[:2], v.part_keys[:2])
    for partials in (v.partials[:2], [v.partials[0], RP._put((RP._get256(v.partials[1]) + 1) % N)]):
        per, verdict = RP.excess_part_verify_host(be, st, two[1], two[2], partials, v.msgs[0])
        assert per == [OK, OK if partials[1] == v.partials[1] else PW.MISMATCH]
        assert PW._plain(tw.excess_part_verify(*two, partials, v.msgs[:1])) == PW._plain([per, [verdict]])


@pytest.mark.parametrize("name", BAL_NAMES)
def test_half_aggregate(arena, oracle_lib, balance_handles, name):
    """d_agg is 33 n + 32 bytes: 65, 98 and 2177 at n = 1, 2, 65 - never a multiple of 16 at these counts"""
    nat, ec = balance_handles[name], oracle_lib
    be, st = OracleBackend(ec), CO._case(ec, name)[0]
    v, A = _job(ec, name, 65).v, arena(1 << 20)
    tw = Twin(nat, A)
    for n in (1, 2, 65):
        keys, msgs, sigs = v.keys[:n], v.msgs[:n], v.sigs[:n]                # host-made keys and signatures of the job of 65 sums
        agg = RP.excess_halfagg_host(b"", keys, msgs, sigs)
        assert len(agg) == 33 * n + 32 and len(agg) % 16
        assert tw.excess_halfagg(keys, msgs, sigs, want_status=True) == (agg, [OK] * n), n
        assert tw.excess_halfagg_verify(keys, msgs, agg, want_status=True, want_point=True) == (True, [OK] * n, None), n
        bent = agg[:-1] + bytes([agg[-1] ^ 1])
        assert tw.excess_halfagg_verify(keys, msgs, bent, want_status=True, want_point=True) == RP.excess_halfagg_verify_host(be, st, keys, msgs, bent, b""), n
    covered(A, "test_half_aggregate")


# ----------------------------------------------------------------------------- 4. verifiers and blocks: nothing in HBM is theirs to write
VERIFY_KEYS = [("flag", "NL"), ("binary two bits", "NL"), ("64bit", None)]


def _host_verdict(ec, key, cf, pf, amounts=None, binding=b""):
    """(status, committed point) of one pair of files by the host protocol code over the oracle: MALFORMED when a coordinate has no curve point"""
    st, binary = PW._host_setup(ec, key)
    mod, nrp = (BRP if binary else RP), (2 if binary else 4)
    if amounts is not None:
        st = with_public(st, key[0], amounts)
    L, lift = Layout(PW._shape(st, binary, cf, pf), nrp), Lift(ec)
    coms = E.decode_commitments(L.nr, cf, lift.many)
    proof = None if coms is None else E.decode_proof(nrp, st.rounds, st.final_lens, coms[0], pf, lift.many)
    if proof is None:
        return MALFORMED, None
    ok = bool(mod.verify(st, proof, RP.sha256_oracle(binding)))
    assert ok == (st.backend.last is None)
    return (VALID if ok else INVALID), st.backend.last


def _raw_batch(A, nat, B, dc, dp, fn="bppp_rp_verify_batch_device"):
    acc, out, st = C.c_int(0), np.zeros(8, dtype=np.uint64), np.zeros(max(B, 1), dtype=np.uint32)
    sd, p = np.frombuffer(SEED, dtype=np.uint8), C.c_void_p
    A.gpu._check(getattr(A.lib, fn)(nat.h, B, p(dc), p(dp), p(sd.ctypes.data), C.byref(acc), p(st.ctypes.data), None, p(out.ctypes.data)), fn)
    return bool(acc.value), [int(s) for s in st[:B]], array_to_point(out)


def _raw_each(A, nat, B, dc, dp):
    st, xy, p = np.zeros(max(B, 1), dtype=np.uint32), np.zeros((max(B, 1), 8), dtype=np.uint64), C.c_void_p
    A.gpu._check(A.lib.bppp_rp_verify_each_device(nat.h, B, p(dc), p(dp), p(st.ctypes.data), p(xy.ctypes.data)), "bppp_rp_verify_each_device")
    return [int(s) for s in st[:B]], [array_to_point(xy[b]) for b in range(B)]


def _no_point(ec, key, cf):
    """the commitments file with its first x replaced by one that has no curve point"""
    nr = len(PW._host_setup(ec, key)[0].rds)
    return CO._set_x(cf, nr, 0, CO._no_point_x(ec))


@pytest.mark.parametrize("key", VERIFY_KEYS, ids=lambda k: k[0])
def test_verifiers(arena, gpu, oracle_lib, nats, key):
    """the honest files of a host proof and its single-field mutants, at 1, 3 and 65 files (file b of a long batch is number b mod the pool), then with
    one file whose first commitment has no curve point: the decode-failure path.  Files of 33 and 418 bytes on 64bit."""
    ec, nat = oracle_lib, nats(key, host_oracle_max=0)
    other = nats(VERIFY_KEYS[(VERIFY_KEYS.index(key) + 1) % 3], host_oracle_max=0)
    files, status, pts, _ = PW._verifier_case(key, 0, None)
    ofiles, ostatus, _, _ = PW._verifier_case(VERIFY_KEYS[(VERIFY_KEYS.index(key) + 1) % 3], 0, 3)
    A = arena(2 << 20)
    for B, malformed in ((1, None), (3, None), (65, None), (3, 1), (65, 64)):
        pick = [b % len(files) for b in range(B)]
        cf, pf = [files[i][0] for i in pick], [files[i][1] for i in pick]
        want_s, want_p = [status[i] for i in pick], [pts[i] for i in pick]
        if malformed is not None:
            cf[malformed] = _no_point(ec, key, cf[malformed])
            assert _host_verdict(ec, key, cf[malformed], pf[malformed]) == (MALFORMED, None)
            want_s[malformed], want_p[malformed] = MALFORMED, None
        ok = all(s == VALID for s in want_s)
        dc, dp = A.to_device(_bytes(cf)), A.to_device(_bytes(pf))
        acc, st, comb = _raw_batch(A, nat, B, dc, dp)
        assert (acc, st) == (ok, want_s), (B, malformed)
        if B <= 3 and malformed is None:
            assert comb == PW._verifier_case(key, 0, B)[3]          # the weighted sum of the host verifier's points
        assert _raw_each(A, nat, B, dc, dp) == (want_s, want_p), (B, malformed)
        with routed(A, nat):
            assert nat.verify_batch_device(B, dc, dp, SEED, want_status=True)[:2] == (ok, want_s)      # the _pub entry points, no amounts given
            assert nat.verify_each_device(B, dc, dp, want_points=True) == (want_s, want_p)
        # two setups in one job
        oc, op = A.to_device(_bytes([c for c, _ in ofiles])), A.to_device(_bytes([p for _, p in ofiles]))
        acc, st, _ = RP.verify_mixed_device(A, [(nat, B, dc, dp), (other, 3, oc, op)], SEED)
        assert (acc, st) == (ok and all(s == VALID for s in ostatus), want_s + ostatus)
        A.check(outputs=[])
    covered(A, "test_verifiers")


def test_verifiers_bound_and_public(arena, gpu, oracle_lib, nats):
    """bindings and per-proof public amounts in HBM: one proof under another's binding, one under another's amount"""
    ec, A = oracle_lib, arena(2 << 20)
    # ---- bindings, on files of 33 and 418 bytes
    key = ("64bit", None)
    nat = nats(key, host_oracle_max=0)
    bind = [hashlib.sha256(b"guarded verify binding %d" % j).digest() for j in PROVE_JS]
    files = PW.host_files(key, PROVE_JS, bindings=tuple(bind))
    for B in COUNTS:
        pick = [b % 3 for b in range(B)]
        given = [bind[i] for i in pick]
        if B > 1:
            given[1] = bind[2]                                      # proof 1 under the binding of proof 2
        cf, pf = [files[i][0] for i in pick], [files[i][1] for i in pick]
        verdicts = [_host_verdict(ec, key, c, p_, binding=g) for c, p_, g in zip(cf, pf, given)]
        want_s, want_p = [s for s, _ in verdicts], [e for _, e in verdicts]
        assert want_s == [INVALID if B > 1 and b == 1 else VALID for b in range(B)]
        dc, dp, db = A.to_device(_bytes(cf)), A.to_device(_bytes(pf)), A.to_device(_bytes(given))
        with routed(A, nat):
            assert nat.verify_batch_device(B, dc, dp, SEED, want_status=True, bindings=db)[:2] == (B == 1, want_s)
            assert nat.verify_each_device(B, dc, dp, want_points=True, bindings=db) == (want_s, want_p)
        A.check(outputs=[])
    # ---- per-proof public amounts
    key = ("flag typed", "NL")
    nat = nats(key, host_oracle_max=0)
    files = PW.host_files(key, PROVE_JS, vary=True)
    for B in COUNTS:
        js = [PROVE_JS[b % 3] for b in range(B)]
        amounts = [PW._amounts(key, j, True) for j in js]
        if B > 1:
            amounts[1] = PW._amounts(key, js[2], True)              # proof 1 under the amount of proof 2
        cf, pf = [files[b % 3][0] for b in range(B)], [files[b % 3][1] for b in range(B)]
        verdicts = [_host_verdict(ec, key, c, p_, amounts=a) for c, p_, a in zip(cf, pf, amounts)]
        want_s, want_p = [s for s, _ in verdicts], [e for _, e in verdicts]
        assert want_s == [INVALID if B > 1 and b == 1 else VALID for b in range(B)]
        pubs = [[PW.public_amount(key[0], a)] for a in amounts]
        dc, dp, da = A.to_device(_bytes(cf)), A.to_device(_bytes(pf)), A.to_device(nat._public_words(pubs, B))
        with routed(A, nat):
            assert nat.verify_batch_device(B, dc, dp, SEED, want_status=True, public_amounts=da)[:2] == (B == 1, want_s)
            assert nat.verify_each_device(B, dc, dp, want_points=True, public_amounts=da) == (want_s, want_p)
        A.check(outputs=[])
    assert {"bppp_rp_verify_batch_pub_device", "bppp_rp_verify_each_pub_device"} <= A.called
    covered(A, "test_verifiers_bound_and_public")


BLOCK_JS = (30, 31, 32, 33)                                        # four host proofs a setup; proof b of a block is number b mod 4


@pytest.mark.parametrize("name", BAL_NAMES)
def test_blocks(arena, gpu, oracle_lib, nats, name):
    """blocks of 1, 4 and 65 proofs, each with unproven rows behind them, three sums and three keys: an honest block, which is then checked again with
    the half-aggregate of its signatures in their place, and (from two proofs on) a block with one wrong member in every part.  The builder is
    test_gpu_poisoned_workspace._block_job, whose sums gather a proven and an unproven row each: a block has two rows at least."""
    ec, nat = oracle_lib, nats((name, None), host_oracle_max=0)
    A = arena(4 << 20)
    for nproofs, rows, salt in ((1, [16], 3), (4, list(range(0, 8)), 1), (65, list(range(8, 16)), 2)):
        js = [BLOCK_JS[b % 4] for b in range(nproofs)]
        for wrong in (False, True)[:1 if nproofs == 1 else 2]:
            args, want = PW._block_job(ec, name, js, rows, salt, wrong)
            with routed(A, nat):
                assert PW._plain(nat.verify_block_device(*args, seed=PW.BAL_SEED, want_status=True)) == want, (nproofs, wrong)
            A.check(outputs=[])
            if not wrong:
                coms, proofs, ss, en, claims, ks, keys, msgs, sigs = args
                agg = RP.excess_halfagg_host(b"", keys, msgs, sigs)
                with routed(A, nat):
                    got = nat.verify_block_agg_device(coms, proofs, ss, en, claims, ks, keys, msgs, agg, seed=PW.BAL_SEED, want_status=True)
                assert PW._plain(got) == want, nproofs
                A.check(outputs=[])
    covered(A, "test_blocks")


# ----------------------------------------------------------------------------- 5. sealed outputs
@pytest.mark.parametrize("name", SS.NAMES)
def test_seal_and_scan(arena, oracle_lib, balance_handles, name):
    """a seal is 34 + 64 * 3 = 226 bytes: 226, 14238 and 14690 bytes at 1, 63 and 65 rows, none a multiple of 16; blindings and openings are 32-byte
    scalars"""
    D, nat = SS._data(oracle_lib, name), balance_handles[name]
    nr, sb = D["nr"], RP.SEAL_BYTES(D["nr"])
    A = arena(2 << 20)
    for rows in (1, 63, 65):
        amt = scalars_to_array([v % 2**256 for row in D["outputs"][:rows] for v, _ in row])
        typ = scalars_to_array([t for row in D["outputs"][:rows] for _, t in row])
        d_vk, d_eph, d_amt = A.to_device(_bytes(D["view_keys"][:rows])), A.to_device(scalars_to_array(D["eph"][:rows])), A.to_device(amt)
        d_typ = A.to_device(typ) if D["typed"] else 0
        d_seals, d_blinds = A.alloc(rows * sb), A.alloc(rows * nr * 32)
        assert (rows * sb) % 16
        with routed(A, nat):
            st = nat.seal_device(rows, d_vk, d_eph, d_amt, d_typ, d_seals, d_blinds, want_status=True)
        assert list(st) == [0] * rows and A.rows(d_seals, rows, sb) == D["seals"][:rows], rows
        assert array_to_scalars(A.download(d_blinds, (rows * nr, 4))) == [x for row in D["blinds"][:rows] for x in row], rows
        A.check(outputs=[d_seals, d_blinds])
        # the scan of the damaged rows: verdicts on the host, three arrays of openings in HBM
        want = D["want"][:rows]
        d_cf, d_sl = A.to_device(_bytes(D["scan_files"][:rows])), A.to_device(_bytes(D["scan_seals"][:rows]))
        outs = [A.alloc(rows * nr * 32) for _ in range(3)]
        with routed(A, nat):
            st, n_own = nat.scan_device(D["a"], rows, d_cf, d_sl, *outs)
        assert list(st) == [v for v, _ in want] and n_own == [v for v, _ in want].count(SS.OWNED), rows
        v, t, bl = (array_to_scalars(A.download(o, (rows * nr, 4))) for o in outs)
        assert [[(v[b * nr + i], t[b * nr + i], bl[b * nr + i]) for i in range(nr)] for b in range(rows)] == [o for _, o in want], rows
        A.check(outputs=outs)
    covered(A, "test_seal_and_scan")


@functools.lru_cache(maxsize=None)
def _scan_singles(name, nkeys):
    """keys a, other, a, then seeded secrets that own nothing, and (statuses, openings) of rangeproof.scan_host under each over the first 65 rows"""
    ec = O.CEC()
    D, be = SS._data(ec, name), OracleBackend(ec)
    rng = random.Random("guarded scan keys " + name)
    keys = [D["a"], D["other"], D["a"]] + [rng.randrange(1, N) for _ in range(nkeys - 3)]
    single = []
    for k in keys:
        res = D["want"][:65] if k == D["a"] else [RP.scan_host(be, D["st"], k, f, s) for f, s in zip(D["scan_files"][:65], D["scan_seals"][:65])]
        single.append(([v for v, _ in res], [o for _, o in res]))
    return keys, single


@pytest.mark.parametrize("name", SS.NAMES)
def test_scan_keys(arena, oracle_lib, balance_handles, name):
    """rows 1, 63, 65 under 1, 2 and KT + 1 keys (KT: the key tile of the geometry hook); the hit list's three arrays of openings have room for the
    hits and one slot more, which the call zeroes"""
    D, nat = SS._data(oracle_lib, name), balance_handles[name]
    nr, KT = D["nr"], SK._geometry(nat, 257, 2**20)[1]
    keys, single = _scan_singles(name, KT + 1)
    A = arena(4 << 20)
    vp, p = (lambda x: C.c_void_p(x.ctypes.data)), C.c_void_p
    for rows in (1, 63, 65):
        for nk in (1, 2, KT + 1):
            want = SK._want(single, nk, rows)
            cap = len(want[1]) + 1
            sec = scalars_to_array(keys[:nk])
            d_cf, d_sl = A.to_device(_bytes(D["scan_files"][:rows])), A.to_device(_bytes(D["scan_seals"][:rows]))
            outs = [A.alloc(cap * nr * 32) for _ in range(3)]
            status, hk, hr = np.full(rows, 0xA5A5A5A5, dtype=np.uint32), np.full(cap, 0xA5A5A5A5, dtype=np.uint32), np.full(cap, 0xA5A5A5A5, dtype=np.uint32)
            nhits, ntag = C.c_size_t(12345), C.c_uint64(12345)
            rc = A.lib.bppp_rp_scan_keys_device(nat.h, nk, vp(sec), rows, p(d_cf), p(d_sl), vp(status), cap, vp(hk), vp(hr), *(p(o) for o in outs), C.byref(nhits), C.byref(ntag))
            v, t, bl = (array_to_scalars(A.download(o, (cap * nr, 4))) for o in outs)
            openings = [[(v[h * nr + i], t[h * nr + i], bl[h * nr + i]) for i in range(nr)] for h in range(cap)]
            SK._check((rc, [int(s) for s in status], [int(x) for x in hk], [int(x) for x in hr], openings, int(nhits.value), int(ntag.value)), want, cap, nr)
            A.check(outputs=outs)
    covered(A, "test_scan_keys")


# ----------------------------------------------------------------------------- 6. cut-through
@pytest.fixture(scope="module")
def cut_handles(gpu, oracle_lib):
    made = {}
    for name in ("64bit", "bin_test"):
        schema = json.load(open(os.path.join(EXAMPLES, name, "schema.json")))
        binary = bool(schema.get("binary"))
        st = (BRP if binary else RP).setup_from_schema(OracleBackend(oracle_lib), schema)
        made[name] = (BRP.NativeBinaryRangeProofs if binary else RP.NativeRangeProofs)(gpu, st)
    yield made
    tl = capi.load_test_library()
    for nat in made.values():
        tl.bppp_test_rp_cut_through_force(nat.h, 0, None, 0)
        nat.close()


def _cut(A, nat, key, j, mode=0, salt=None, bits=0):
    """one job through bppp_rp_cut_through_device against rangeproof.cut_through_host; the new pool has rows * coms_bytes bytes and the new entries
    4 * nnz, as include/bppp.h sizes them, whatever survives"""
    want = CT._want(nat, key, j)
    CT._force(nat, mode, salt, bits)
    try:
        with routed(A, nat):
            got = CT._run(nat, j, True, alloc=A)
    finally:
        CT._force(nat)
    CT._same(got, want)
    (d_pool, n_pool), (d_en, n_en) = A.buffer_ranges()[-2:]
    assert (n_pool, n_en) == (len(j["rows"]) * nat.shape["coms_bytes"], 4 * len(j["entries"]))
    A.check(outputs=[d_pool, d_en])


@pytest.mark.parametrize("handle", ["64bit", "bin_test"])
def test_cut_through(arena, cut_handles, handle):
    """rows of 33 bytes (64bit) and 97 bytes (bin_test): the 16-byte-wide gather of the new pool ends in a short chunk at nearly every size; the new
    entries are 4 bytes each, 4 bytes in all at nnz = 1"""
    nat, A = cut_handles[handle], arena(4 << 20)
    shape = (lambda j: j) if handle == "64bit" else (lambda j: CJ.widen(j, 3))
    for key, j in CJ.hand_made().items():
        _cut(A, nat, ("guarded", handle, key), shape(j))
    for nnz in (1, 65, 257):
        j = shape(CJ.random_job(1000 + nnz, nnz))
        assert len(j["entries"]) == nnz
        _cut(A, nat, ("guarded rnd", handle, nnz), j)
    _cut(A, nat, ("guarded rnd", handle, 65), shape(CJ.random_job(1065, 65)), mode=1, salt=CT.SALTS[0], bits=1)      # every hash equal, the smallest table
    covered(A, "test_cut_through")
