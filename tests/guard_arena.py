"""An arena allocator with guard bands for the device-call tests (no tests in this file).

include/bppp.h promises callers of the d_* parameters "HBM-resident, 16-byte aligned" and nothing more.  A GuardArena takes ONE allocation from
the object it is given, fills it with a guard byte and hands out sub-buffers that are exactly as long as asked, start at an address = 16 (mod 256)
- 16-byte alignment and nothing stronger - and are fenced by guard bytes: at least 1 KiB before the first buffer and between neighbours, at least
64 KiB behind the last one.  check() downloads the arena once and asserts that every guard byte still holds the guard value and that every buffer
marked as an input still holds the bytes the host uploaded to it.

The arena offers what the tests' device helpers use of a context - alloc, to_device, upload, download, free (a no-op) - and reaches memory only
through alloc / upload / download / free of the object it is given, so a host-only fake can stand in for the GPU (test_guard_arena_host.py)."""
import numpy as np

GUARD = 0x5C                 # none of 0x00 (zeroed outputs), 0xA5 (the poison byte), 0xFF (CUT_NONE words): those would hide a write of the suite's own values
PHASE, PERIOD = 16, 256      # every buffer starts at an address = PHASE (mod PERIOD)
GAP = 1024                   # least guard before the first buffer and between neighbours
TAIL = 64 * 1024             # least guard behind the last buffer: a long overrun still lands in memory the arena owns


class GuardError(AssertionError):
    """what check() found: the buffer's name, the side ("before", "after" or "input") and the first and last offending offset, relative to the
    buffer's first byte (negative before it)"""

    def __init__(self, buffer, side, first, last, count, index):
        self.buffer, self.side, self.first, self.last, self.count, self.index = buffer, side, first, last, count, index
        what = "a const input changed" if side == "input" else "guard bytes %s the buffer changed" % side
        super().__init__("%s: %s, %d byte(s), offsets %d .. %d from the buffer's start" % (buffer, what, count, first, last))


class GuardArena:
    def __init__(self, gpu, capacity_bytes):
        self.gpu, self.capacity = gpu, int(capacity_bytes)
        assert self.capacity >= GAP + PERIOD + TAIL
        self.base = gpu.alloc(self.capacity)
        gpu.upload(self.base, np.full(self.capacity, GUARD, dtype=np.uint8))
        self.bufs = []                                             # [offset, nbytes, name, host mirror, marked copy or None]
        self._by_ptr, self._outputs = {}, set()

    def close(self):
        if self.base:
            self.gpu.free(self.base)
            self.base = 0

    # ---- the allocator's surface
    def alloc(self, nbytes, name=None):
        nbytes = int(nbytes)
        assert nbytes >= 0
        end = self.bufs[-1][0] + self.bufs[-1][1] if self.bufs else 0
        off = end + GAP
        off += (PHASE - (self.base + off)) % PERIOD
        if off + nbytes + TAIL > self.capacity:
            raise MemoryError("GuardArena of %d bytes is full: %d buffers, %d more bytes asked" % (self.capacity, len(self.bufs), nbytes))
        name = "buffer %d%s [%d bytes]" % (len(self.bufs), " '%s'" % name if name else "", nbytes)
        self._by_ptr[self.base + off] = len(self.bufs)
        self.bufs.append([off, nbytes, name, np.full(nbytes, GUARD, dtype=np.uint8), None])
        return self.base + off

    def to_device(self, arr, name=None):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes, name)
        if arr.nbytes:
            self.upload(p, arr)
        return p

    def upload(self, d_dst, src):
        src = np.ascontiguousarray(src)
        raw = src.reshape(-1).view(np.uint8)
        i, at = self._find(d_dst)
        assert at + raw.size <= self.bufs[i][1], "upload of %d bytes at +%d runs over %s" % (raw.size, at, self.bufs[i][2])
        self.gpu.upload(d_dst, src)
        self.bufs[i][3][at:at + raw.size] = raw

    def download(self, d_src, shape, dtype=np.uint64):
        return self.gpu.download(d_src, shape, dtype)

    def free(self, d_ptr):
        pass

    # ---- the checks
    def _find(self, ptr):
        """(index of the buffer that holds address ptr, offset in it)"""
        if ptr in self._by_ptr:
            return self._by_ptr[ptr], 0
        for i, (off, n, *_) in enumerate(self.bufs):
            if self.base + off <= ptr < self.base + off + n:
                return i, ptr - self.base - off
        raise KeyError("0x%x is in no buffer of this arena" % ptr)

    def mark_input(self, ptr):
        """the buffer at ptr is a `const` input of the call: check() compares it with what the host uploaded to it"""
        i, at = self._find(ptr)
        assert at == 0
        self.bufs[i][4] = self.bufs[i][3].copy()

    def mark_inputs(self, exclude=()):
        """every buffer but those at the pointers in `exclude` (the call's outputs) is an input"""
        skip = {self._find(p)[0] for p in exclude if p}
        for i, b in enumerate(self.bufs):
            b[4] = None if i in skip else b[3].copy()

    def check(self, outputs=None):
        """one download; GuardError for the first buffer with a changed guard byte around it or, marked as an input, a changed byte in it.
        outputs: the pointers the call may write; then every buffer that no check of this arena has named as an output is marked first"""
        if outputs is not None:
            self._outputs |= {p for p in outputs if p}
            self.mark_inputs(exclude=self._outputs)
        got = self.gpu.download(self.base, (self.capacity,), np.uint8)
        bad = got != GUARD
        for off, n, *_ in self.bufs:
            bad[off:off + n] = False
        if bad.any():
            where = np.flatnonzero(bad)
            starts = np.array([b[0] for b in self.bufs], dtype=np.int64)
            ends = np.array([b[0] + b[1] for b in self.bufs], dtype=np.int64)
            o = int(where[0])
            if not self.bufs:
                raise GuardError("the empty arena", "after", o, int(where[-1]), where.size, -1)
            nxt = int(np.searchsorted(starts, o, side="right"))    # the first buffer that starts above o; the one below it ends at or below o
            lo = int(ends[nxt - 1]) if nxt else 0                  # the gap that holds o: [lo, hi)
            hi = int(starts[nxt]) if nxt < len(self.bufs) else self.capacity
            gap = where[(where >= lo) & (where < hi)]
            # a byte of the gap belongs to the nearer neighbour: "after" the buffer below it, "before" the one above (a tie goes below)
            below = np.ones(gap.size, dtype=bool) if nxt == len(self.bufs) else np.zeros(gap.size, dtype=bool) if nxt == 0 else gap - lo <= hi - 1 - gap
            i, side = (nxt - 1, "after") if below[0] else (nxt, "before")
            mine = gap[below == below[0]]
            raise GuardError(self.bufs[i][2], side, int(mine[0]) - int(starts[i]), int(mine[-1]) - int(starts[i]), int(mine.size), i)
        for i, (off, n, name, _, marked) in enumerate(self.bufs):
            if marked is not None:
                diff = np.flatnonzero(got[off:off + n] != marked)
                if diff.size:
                    raise GuardError(name, "input", int(diff[0]), int(diff[-1]), int(diff.size), i)

    def buffer_ranges(self):
        """[(address, nbytes)] of the buffers handed out, in order"""
        return [(self.base + off, n) for off, n, *_ in self.bufs]
