"""A GuardArena whose memory arrives late, on a caller's busy stream (helper, no tests in this file).

include/bppp.h makes two promises about streams: a context bound with bppp_ctx_set_stream runs all its work on the caller's stream, so the producers
of a d_* input may still be queued on that stream when the library is called; and every call is synchronous on return, so nothing of it is in flight
on any stream afterwards.  The pieces here put both under load for every call that goes through an arena:

  LateWorld    one per test module: a context of its own (capi.Bppp) bound to a torch side stream `s`, a second side stream for off-stream reads, a
               calibrated delay (plain torch elementwise operations over a scratch tensor) and the counters of the whole module.
  TorchMemory  what a GuardArena takes for its `gpu`: alloc / upload / download / free over torch uint8 tensors, everything else (h, lib, _check, ...)
               forwarded to the world's context.  The arena's one allocation is one tensor; guard bands, phase 16 mod 256 and check() are GuardArena's.
  LateArena    test_gpu_guarded_outputs.ArenaGpu over a TorchMemory; its `lib` is a LateRecorder.
  LateRecorder the library, with the late world around every symbol called through it:
                 1. hide: drain s, copy the arena to a shadow tensor, zero the arena, drain.  Zero is scalar 0, the point at infinity, index 0, an
                    empty CSR: every entry point judges these without reading out of bounds, so a read that runs ahead of the stream gives a clean
                    wrong answer or a refusal;
                 2. deliver late: on s the delay, behind it the copy shadow -> arena, then an event E.  Whatever the call may read - uploaded by the
                    host or written by an earlier call - arrives behind the delay;
                 3. late = not E.query() immediately before the call: a call that was not late tested nothing and is counted;
                 4. on return, before any synchronisation, the arena is copied to the host on the reader stream, which waits on nothing (R1); then s
                    is drained and the arena copied again (R2).  R1 == R2 byte for byte, for failing return codes too, or StreamOrderError names the
                    symbol, the offsets and the buffer;
                 5. a symbol that was called late and checked on return goes into world.late_called.

One departure from "every symbol alike", and why.  A call that takes no device memory (bppp_rp_info, bppp_last_error, bppp_basis_create from host
points, ...) has no reason to wait for the caller's stream, and when it returns at once the delivery of step 2 - the harness's own, not the call's -
is still queued: R1 would be the zeroed arena and R2 the restored one.  So for a symbol that is NOT an entry point of the guarded CASES table, step 4
is skipped when E is still pending on return; the symbol is noted in world.returned_early.  For the CASES entry points there is no such way out: they
read or write device memory, their last act is a drain of the bound stream, and that drain has to cover the delivery queued in front of them."""
import time

import numpy as np

from guard_arena import GuardError
from test_gpu_guarded_outputs import CASES, ArenaGpu

DELAY_FLOOR_MS = 2.0         # the delay is 20 times the measured host gap at least, and this long at least: long enough that the library's first reads
                             # of a call (tens to hundreds of microseconds after entry) fall well inside it
SCRATCH_FLOATS = 1 << 26     # the delay's scratch tensor, 256 MiB: one in-place operation over it streams 512 MiB through HBM, on the order of 0.1 ms
NOT_LATE_CAP = 0.05          # at most this share of the recorded calls may have been entered with the delivery already complete


class StreamOrderError(AssertionError):
    """the arena as read off-stream on return (R1) differs from the arena after the bound stream drained (R2)"""

    def __init__(self, symbol, rc, drained, buffer, first, last, count):
        self.symbol, self.rc, self.drained, self.buffer, self.first, self.last, self.count = symbol, rc, drained, buffer, first, last, count
        state = "had arrived" if drained else "was still queued"            # `drained`: E, recorded behind the delivery, was complete on return
        super().__init__("%s (returned %d) returned with work in flight on the bound stream (the late delivery in front of it %s): device memory changed "
                         "after the return - %s: %d byte(s), offsets %d .. %d from the buffer's start" % (symbol, rc, state, buffer, count, first, last))


class LateWorld:
    def __init__(self, device=0, reader="side"):
        import torch
        import bulletproofspp_amd as b
        self.torch, self.dev = torch, torch.device("cuda", device)
        self.s, self.s2 = torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev)
        self.reader_name = reader
        self.reader = self.s2 if reader == "side" else torch.cuda.default_stream(self.dev)      # "null": torch's default stream is the null stream
        self.ctx = b.Bppp(device)
        self.ctx.set_stream(self.s.cuda_stream)
        self.event = torch.cuda.Event()
        self.scratch = torch.zeros(SCRATCH_FLOATS, dtype=torch.float32, device=self.dev)
        self._bufs = {}                                            # capacity -> (shadow tensor, pinned R1, pinned R2)
        self.late_called, self.returned_early = set(), set()
        self.calls, self.not_late, self.not_late_symbols, self.gaps_us = 0, 0, [], []
        self.t0 = time.perf_counter()
        self._calibrate()

    def close(self):
        if self.ctx is not None:
            self.torch.cuda.synchronize(self.dev)
            self.ctx.close()
            self.ctx = None
            self.scratch, self._bufs = None, {}

    # ---- the delay
    def _calibrate(self):
        """op_ms: one scratch operation on the idle stream, by HIP events; gap_us: the host time from just before recording E to the point where the
        library call is entered, the worst of 200 dry runs of exactly those statements; delay_ops: what makes the delay 20 gaps and DELAY_FLOOR_MS
        long at least; delay_ms: that delay as then measured"""
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(ops):
            self.s.synchronize()
            with torch.cuda.stream(self.s):
                e0.record(self.s)
                for _ in range(ops):
                    self.scratch.add_(1.0)
                e1.record(self.s)
            self.s.synchronize()
            return e0.elapsed_time(e1)
        timed(4)                                                   # first launches: code load, allocator
        self.op_ms = timed(16) / 16
        gaps = []
        for _ in range(200):
            with torch.cuda.stream(self.s):
                t0 = time.perf_counter()
                self.event.record(self.s)
            late = not self.event.query()
            gaps.append((time.perf_counter() - t0) * 1e6)
        self.s.synchronize()
        self.gap_us = max(gaps[1:])
        want_ms = max(DELAY_FLOOR_MS, 20 * self.gap_us / 1e3)
        self.delay_ops = int(np.ceil(want_ms / self.op_ms))
        assert self.delay_ops <= 512, "a delay of %.2f ms from operations of %.4f ms: the calibration is off" % (want_ms, self.op_ms)
        self.delay_ms = timed(self.delay_ops)
        assert self.delay_ms * 1e3 >= 20 * self.gap_us, (self.delay_ms, self.gap_us)

    def delay(self):
        """enqueue the delay on the current stream"""
        for _ in range(self.delay_ops):
            self.scratch.add_(1.0)

    # ---- per-size staging, shared by the arenas of the module
    def staging(self, nbytes):
        if nbytes not in self._bufs:
            torch = self.torch
            self._bufs[nbytes] = (torch.empty(nbytes, dtype=torch.uint8, device=self.dev), torch.empty(nbytes, dtype=torch.uint8, pin_memory=True),
                                  torch.empty(nbytes, dtype=torch.uint8, pin_memory=True))
        return self._bufs[nbytes]

    def read_off_stream(self, tensor, out):
        """copy `tensor` to the pinned host tensor `out` on the reader stream, which waits on nothing; wait for that copy alone"""
        with self.torch.cuda.stream(self.reader):
            out.copy_(tensor, non_blocking=True)
        self.reader.synchronize()

    def read_in_order(self, tensor, out):
        self.s.synchronize()
        with self.torch.cuda.stream(self.s):
            out.copy_(tensor, non_blocking=True)
        self.s.synchronize()

    def hide_and_deliver_late(self, tensor):
        """steps 1 and 2 for one tensor; returns with E recorded behind the delivery, and the host's clock from just before that record"""
        torch, (shadow, _, _) = self.torch, self.staging(tensor.numel())
        self.s.synchronize()
        with torch.cuda.stream(self.s):
            shadow.copy_(tensor)
            tensor.zero_()
        self.s.synchronize()
        with torch.cuda.stream(self.s):
            self.delay()
            tensor.copy_(shadow)
            t_record = time.perf_counter()
            self.event.record(self.s)
        return t_record

    def report(self):
        gaps = sorted(self.gaps_us) or [0.0]
        return ("late world: reader %s, %d recorded calls, %d not late %s; host gap calibrated %.1f us (in the calls: median %.1f, max %.1f us); "
                "delay %d operations of %.3f ms = %.2f ms; %.1f s since the module's setup; returned before the delivery, no device memory: %s"
                % (self.reader_name, self.calls, self.not_late, sorted(set(self.not_late_symbols)), self.gap_us, gaps[len(gaps) // 2], gaps[-1],
                   self.delay_ops, self.op_ms, self.delay_ms, time.perf_counter() - self.t0, sorted(self.returned_early)))


class TorchMemory:
    """alloc / upload / download / free over torch uint8 tensors on the world's stream; every other attribute is the world's context's"""

    def __init__(self, world):
        self.world, self.tensors = world, {}

    def __getattr__(self, name):
        return getattr(self.__dict__["world"].ctx, name)

    def alloc(self, nbytes):
        w = self.world
        t = w.torch.empty(max(int(nbytes), 16), dtype=w.torch.uint8, device=w.dev)
        w.torch.cuda.synchronize(w.dev)                            # the allocator may hand out memory another stream used last
        self.tensors[t.data_ptr()] = t
        return t.data_ptr()

    def free(self, d_ptr):
        self.world.s.synchronize()
        del self.tensors[d_ptr]

    def _slice(self, ptr, nbytes):
        """the nbytes bytes at device address ptr, which may lie anywhere inside one of the tensors: a view of it"""
        for base, t in self.tensors.items():
            if base <= ptr and ptr + nbytes <= base + t.numel():
                return t[ptr - base:ptr - base + nbytes]
        raise KeyError("%d bytes at 0x%x are in no tensor of this memory" % (nbytes, ptr))

    def upload(self, d_dst, src):
        w = self.world
        raw = np.ascontiguousarray(src).reshape(-1).view(np.uint8)
        if raw.size:
            with w.torch.cuda.stream(w.s):
                self._slice(d_dst, raw.size).copy_(w.torch.from_numpy(raw.copy()))
            w.s.synchronize()

    def download(self, d_src, shape, dtype=np.uint64):
        w = self.world
        out = np.zeros(shape, dtype=dtype)
        if out.nbytes:
            with w.torch.cuda.stream(w.s):
                host = self._slice(d_src, out.nbytes).cpu()
            w.s.synchronize()
            out.reshape(-1).view(np.uint8)[:] = host.numpy()
        return out


class LateRecorder:
    """the library, with the late world around every symbol that is called through it (the module docstring's five steps)"""

    def __init__(self, lib, arena):
        self._lib, self._arena = lib, arena

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        arena = self._arena
        w = arena.world

        def call(*args):
            tensor = arena.gpu.tensors[arena.base]
            _, r1, r2 = w.staging(tensor.numel())
            arena.called.add(name)
            t_record = w.hide_and_deliver_late(tensor)             # ends like the calibration's dry run: record E, leave the stream block, query E
            late = not w.event.query()
            t_enter = time.perf_counter()
            rc = fn(*args)
            w.gaps_us.append((t_enter - t_record) * 1e6)
            drained = w.event.query()
            w.calls += 1
            if not late:
                w.not_late += 1
                w.not_late_symbols.append(name)
            if not drained and name not in CASES:                  # took no device memory and did not wait: what is pending is the harness's own delivery
                w.returned_early.add(name)
                w.s.synchronize()
                return rc
            w.read_off_stream(tensor, r1)
            w.read_in_order(tensor, r2)
            if not w.torch.equal(r1, r2):
                where = np.flatnonzero(r1.numpy() != r2.numpy())
                raise arena.stream_order_error(name, rc, drained, where)
            if late:
                w.late_called.add(name)
            return rc
        return call


class LateArena(ArenaGpu):
    """ArenaGpu over torch memory on the world's busy stream; every library call made through it runs in the late world"""

    def __init__(self, world, capacity_bytes):
        self.world = world
        super().__init__(TorchMemory(world), capacity_bytes)
        self._late = LateRecorder(world.ctx.lib, self)

    @property
    def lib(self):
        return self._late

    def stream_order_error(self, symbol, rc, drained, where):
        """StreamOrderError for the arena offsets `where` (sorted): named after the first buffer that holds any of them (when the whole delivery was
        still queued every byte differs, the guard bands too: the buffer says more), else after the guard band, in GuardError's terms"""
        o = int(where[0])
        for off, n, name, *_ in self.bufs:
            lo, hi = np.searchsorted(where, off), np.searchsorted(where, off + n)
            if hi > lo:
                mine = where[lo:hi]
                return StreamOrderError(symbol, rc, drained, name, int(mine[0]) - off, int(mine[-1]) - off, int(mine.size))
        below = [b for b in self.bufs if b[0] + b[1] <= o]
        if below:
            off, n, name = below[-1][:3]
            return StreamOrderError(symbol, rc, drained, "guard bytes after " + name, o - off, int(where[-1]) - off, int(where.size))
        return StreamOrderError(symbol, rc, drained, "guard bytes before the first buffer", o, int(where[-1]), int(where.size))


__all__ = ["LateWorld", "LateArena", "TorchMemory", "LateRecorder", "StreamOrderError", "GuardError", "NOT_LATE_CAP"]
