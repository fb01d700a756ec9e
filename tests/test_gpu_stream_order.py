"""Every device entry point on a caller's busy stream, its inputs arriving late.

include/bppp.h, at bppp_ctx_set_stream: the d_* inputs of a call may be produced by work that is still queued on the bound stream, and on return
nothing of the call is in flight on any stream.  The library mixes asynchronous copies on the context's stream, plain hipMemcpy on the null stream (which
is ordered against a non-blocking stream by nothing but the hipStreamSynchronize that happens to stand in front of it) and a second stream of its own,
so both promises rest on about sixty entry points each remembering its waits.  This module runs the guarded cases of test_gpu_guarded_outputs.py - the
same functions, parametrisations, oracle comparisons, arena.check() and covered() - with `gpu` and `arena` resolving to a context bound to a torch side
stream and to a LateArena (tests/late_arena.py): around every library call the arena is zeroed and its contents are delivered on the bound stream behind
a delay, the call is entered while that delivery is still pending, and on return the arena is read off-stream before any synchronisation and must equal
what it holds after the stream has drained.

Off-stream reader: the second torch side stream (READER = "side"), which is what test_the_harness_sees_a_race holds: with the process's streams mapped
onto four hardware queues the reader could share a queue with the bound stream and wait behind the delay; the control then fails, since every other
test here would be vacuous.  (The fallback would be READER = "null", a copy on torch's default stream.)

Regression notes (sites in csrc/ that a case of this module caught):
  - csrc/trrp.hip, bppp_trrp_public_device (test_trrp_public, all three batch sizes): the entry point queued its kernels and returned - the header
    called it "asynchronous on the context's stream", the one exception to the ABI's rule - so its five output arrays changed after the return.  It now
    drains the bound stream at its tail (both streams after a refusal); the verifiers inside the library call trrp_public_run and are not affected.
The other 58 entry points of CASES held both promises as measured.

Measured on an MI355X: host gap between recording E and entering a call 4 - 5 us (worst of 200 dry runs; in the calls: median 4.6 us, worst 32 us);
delay 28 scratch operations of 0.073 ms = 2.05 ms (the floor of late_arena.DELAY_FLOOR_MS, 400 gaps); 477 recorded calls, none of them not late;
the module takes 14 - 15 s, its slowest case 1.5 s."""
import random

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads the library: torch's wheel carries a HIP runtime of its own, and only the one loaded
#                           first is shared by both - a stream of one runtime means nothing to the other (tests/test_dist_gloo.py imports it as early)

import pyoracle as O
import test_gpu_guarded_outputs as G
import test_gpu_poisoned_workspace as PW
from bulletproofspp_amd import capi
from bulletproofspp_amd.capi import points_to_array, scalars_to_array
from guard_arena import GuardArena
from late_arena import NOT_LATE_CAP, LateArena, LateWorld
from test_gpu_guarded_outputs import (balance_handles, cut_handles, nats, test_arena_memory_calls, test_argument_verifiers,  # noqa: F401
                                      test_balance_calls, test_batch_inverse, test_blocks, test_cut_through, test_fold_points, test_glv_decompose,
                                      test_half_aggregate, test_lift_x_and_seed_points, test_msm_inputs, test_provers, test_round_scalars, test_scan_keys,
                                      test_seal_and_scan, test_tensor, test_trrp_public, test_verifiers, test_verifiers_bound_and_public)
from test_gpu_verify_each import SEED

pytestmark = pytest.mark.gpu

READER = "side"
N = O.N


@pytest.fixture(scope="module")
def world():
    w = LateWorld(0, READER)
    yield w
    w.close()


@pytest.fixture(scope="module")
def gpu(world):
    """the module's own context, bound to the world's busy stream: the handles of nats, balance_handles and cut_handles are made on it"""
    return world.ctx


@pytest.fixture
def arena(world):
    made = []

    def make(capacity=4 << 20):
        made.append(LateArena(world, capacity))
        return made[-1]
    yield make
    for a in made:
        a.close()


def test_the_guarded_cases_are_all_here():
    """every test CASES names is collected in this module too, as the same function object"""
    assert {name: globals().get(name) for name in set(G.CASES.values())} == {name: getattr(G, name) for name in set(G.CASES.values())}
    assert all(globals()[f] is getattr(G, f) for f in ("nats", "balance_handles", "cut_handles"))


# ----------------------------------------------------------------------------- the control: the library is not involved
def test_the_harness_sees_a_race(world, arena):
    """a pattern, hidden and delivered late: the off-stream reader sees zeros while E is pending, the pattern once the bound stream has drained.  Were
    the first read to show the pattern, the reader would be serialised behind the bound stream and R1 == R2 would hold for any library"""
    A, torch = arena(1 << 18), world.torch
    pattern = np.frombuffer(random.Random("late pattern").randbytes(4099), dtype=np.uint8)
    p = A.to_device(pattern)
    tensor = A.gpu.tensors[A.base]
    off = p - A.base
    _, r1, r2 = world.staging(tensor.numel())
    world.hide_and_deliver_late(tensor)
    pending = not world.event.query()
    world.read_off_stream(tensor, r1)
    still_pending = not world.event.query()
    early = r1.numpy()[off:off + pattern.size].copy()
    early_all = int(np.count_nonzero(r1.numpy()))
    world.read_in_order(tensor, r2)
    assert world.event.query()
    assert pending and still_pending, "the delay of %.2f ms ran out before an off-stream copy of %d bytes returned" % (world.delay_ms, tensor.numel())
    assert early_all == 0 and not early.any(), "the off-stream reader '%s' waited for the bound stream: the streams are serialised" % world.reader_name
    assert r2.numpy()[off:off + pattern.size].tobytes() == pattern.tobytes()
    A.check(outputs=[])
    # the recorder's own error, from two reads that differ in one buffer and in the guard band behind it
    where = np.array([off + 5, off + 9, off + pattern.size + 2])
    err = A.stream_order_error("bppp_example_device", -4, False, where)
    assert (err.symbol, err.rc, err.first, err.last, err.count) == ("bppp_example_device", -4, 5, 9, 2) and "[4099 bytes]" in err.buffer
    assert "bppp_example_device (returned -4)" in str(err) and "2 byte(s), offsets 5 .. 9 from the buffer's start" in str(err)
    err = A.stream_order_error("bppp_example_device", 0, True, where[2:])
    assert err.buffer.startswith("guard bytes after buffer 0") and (err.first, err.count) == (pattern.size + 2, 1)


# ----------------------------------------------------------------------------- bppp_ctx_set_stream itself
def _msm(ctx, ec, seed):
    rnd = random.Random("stream order msm %d" % seed)
    pts = O.hash_points(b"stream order msm", 301)
    sc = [rnd.randrange(N) for _ in range(301)]
    sc[3], pts[5] = 0, None
    ds, dp = ctx.to_device(scalars_to_array(sc)), ctx.to_device(points_to_array(pts))
    try:
        return ctx.msm_device(ds, dp, 301), ec.inner_product(list(zip(sc, pts)))
    finally:
        ctx.free(ds); ctx.free(dp)


def test_set_stream_null_rebinding_and_handles(world, oracle_lib):
    """binding NULL goes back to the context's own stream; rebinding returns only after the stream bound before has drained (capi.hip,
    bppp_ctx_set_stream: the hipStreamSynchronize in front of the assignment); a range-proof handle made before a rebinding works after it"""
    import bulletproofspp_amd as b
    torch, ec = world.torch, oracle_lib
    s, s3 = torch.cuda.Stream(device=world.dev), torch.cuda.Stream(device=world.dev)
    key = ("flag", "NL")
    files, status, _, _ = PW._verifier_case(key, 0, 3)
    cf, pf = [c for c, _ in files], [p for _, p in files]
    ctx = b.Bppp(0)
    try:
        ctx.set_stream(s.cuda_stream)
        got, want = _msm(ctx, ec, 1)
        assert got == want
        nat = PW._native(ctx, ec, key)                              # made while s is bound
        assert tuple(nat.verify_batch(cf, pf, SEED, want_status=True)[:2]) == (False, status)
        # rebinding while a delay is pending on s
        event = torch.cuda.Event()
        with torch.cuda.stream(s):
            world.delay()
            event.record(s)
        pending = not event.query()
        ctx.set_stream(s3.cuda_stream)
        assert event.query(), "bppp_ctx_set_stream returned with the stream it unbound still busy"
        assert pending, "the delay of %.2f ms had run out before the call: nothing was tested" % world.delay_ms
        got, want = _msm(ctx, ec, 2)
        assert got == want
        assert tuple(nat.verify_batch(cf, pf, SEED, want_status=True)[:2]) == (False, status)
        assert tuple(nat.verify_batch(cf[:1], pf[:1], SEED, want_status=True)[:2]) == (True, status[:1])
        # NULL: the context's own stream again, also while the bound stream is busy
        with torch.cuda.stream(s3):
            world.delay()
            event.record(s3)
        ctx.set_stream(0)
        assert event.query()
        got, want = _msm(ctx, ec, 3)
        assert got == want
        assert [int(v) for v in nat.verify_each(cf, pf)] == status
        nat.close()
    finally:
        ctx.close()
        torch.cuda.synchronize(world.dev)


def test_destroy_with_a_bound_stream_then_a_child(world, oracle_lib):
    """bppp_ctx_destroy with a caller's stream bound falls back to the context's own stream for what the children still do (capi.hip,
    bppp_ctx_destroy): destroying a child handle afterwards, with the caller's stream gone, returns without error"""
    import bulletproofspp_amd as b
    torch = world.torch
    s = torch.cuda.Stream(device=world.dev)
    ctx = b.Bppp(0, stream=s.cuda_stream)
    nat = PW._native(ctx, oracle_lib, ("flag", "NL"))
    h_ctx, h_nat = ctx.h, nat.h
    got, want = _msm(ctx, oracle_lib, 4)
    assert got == want
    ctx.lib.bppp_ctx_destroy(h_ctx)                                # the context first: the child keeps it alive
    ctx.h = None
    assert h_nat and nat.h is h_nat
    nat.close()                                                    # bppp_rp_destroy: releases the context's stream and workspaces with the last child
    assert nat.h is None
    torch.cuda.synchronize(world.dev)


# ----------------------------------------------------------------------------- completeness: this test stays last
def test_every_entry_point_was_called_late(world):
    """accumulated over the module: every entry point of CASES was entered at least once while the delivery of its inputs was still pending and was
    checked on return, and at most 5 % of all recorded calls found the delivery already complete"""
    print(world.report())
    assert world.calls > 0
    missing = sorted(set(G.CASES) - world.late_called)
    assert not missing, "never called late: %s" % missing
    assert world.not_late <= NOT_LATE_CAP * world.calls, (world.not_late, world.calls, sorted(set(world.not_late_symbols)))
    assert not set(G.CASES) & world.returned_early
    assert world.delay_ms * 1e3 >= 20 * world.gap_us
