"""tests/guard_arena.py on a bytearray: the arena's placement, its exact lengths, and that check() reports one changed byte at every place where a
kernel's overrun or a written input would show - with the right buffer and side.  No GPU."""
import numpy as np
import pytest

from guard_arena import GAP, GUARD, PERIOD, PHASE, TAIL, GuardArena, GuardError

LENGTHS = [1, 33, 418, 4 * 65, 64, 0, 33 * 65 + 32]


class FakeGpu:
    """alloc / upload / download / free over one bytearray; addresses start at an odd multiple of 4 KiB"""
    BASE = 0x7F0000001000

    def __init__(self):
        self.mem, self.allocs, self.freed, self.downloads = bytearray(), [], [], 0

    def alloc(self, nbytes):
        p = self.BASE + len(self.mem)
        self.mem += bytes(-(-nbytes // 4096) * 4096)
        self.allocs.append((p, nbytes))
        return p

    def free(self, ptr):
        self.freed.append(ptr)

    def upload(self, dst, src):
        raw = np.ascontiguousarray(src).reshape(-1).view(np.uint8).tobytes()
        at = dst - self.BASE
        assert 0 <= at and at + len(raw) <= len(self.mem)
        self.mem[at:at + len(raw)] = raw

    def download(self, src, shape, dtype=np.uint64):
        out = np.zeros(shape, dtype=dtype)
        at = src - self.BASE
        assert 0 <= at and at + out.nbytes <= len(self.mem)
        self.downloads += 1
        return np.frombuffer(bytes(self.mem[at:at + out.nbytes]), dtype=dtype).reshape(shape).copy()

    def poke(self, addr, value):
        self.mem[addr - self.BASE] = value


@pytest.fixture
def arena():
    g = FakeGpu()
    a = GuardArena(g, 1 << 20)
    ptrs = [a.to_device(np.arange(n, dtype=np.uint8)) if k % 2 == 0 else a.alloc(n) for k, n in enumerate(LENGTHS)]
    return g, a, ptrs


def test_one_allocation_filled_with_the_guard_byte():
    g = FakeGpu()
    a = GuardArena(g, 1 << 20)
    assert g.allocs == [(a.base, 1 << 20)] and bytes(g.mem[:1 << 20]) == bytes([GUARD]) * (1 << 20)
    assert GUARD not in (0x00, 0xA5, 0xFF)
    a.check()
    a.free(a.alloc(7))
    assert g.freed == [] and len(g.allocs) == 1                   # free is a no-op; buffers come from the one allocation
    a.close()
    assert g.freed == [a.base or g.allocs[0][0]]


def test_offsets_lengths_and_gaps(arena):
    g, a, ptrs = arena
    assert (PHASE, PERIOD, GAP, TAIL) == (16, 256, 1024, 65536)
    assert a.buffer_ranges() == list(zip(ptrs, LENGTHS))           # exact lengths, nothing rounded up
    for p in ptrs:
        assert p % 256 == 16                                       # 16-byte aligned and nothing stronger
    assert ptrs[0] - a.base >= GAP
    for (p, n), q in zip(zip(ptrs, LENGTHS), ptrs[1:]):
        assert q - (p + n) >= GAP
    assert a.base + a.capacity - (ptrs[-1] + LENGTHS[-1]) >= TAIL
    small = GuardArena(FakeGpu(), GAP + PERIOD + TAIL + 100)
    small.alloc(50)
    with pytest.raises(MemoryError):
        small.alloc(100)                                           # the tail guard is never given away


def test_interior_writes_pass_with_one_download(arena):
    g, a, ptrs = arena
    for p, n in zip(ptrs, LENGTHS):
        if n and p not in (ptrs[0], ptrs[2]):
            g.upload(p, np.full(n, 0xEE, dtype=np.uint8))          # first to last byte of every output
    a.mark_input(ptrs[0]); a.mark_input(ptrs[2])
    before = g.downloads
    a.check()
    assert g.downloads == before + 1
    assert a.download(ptrs[1], (33,), np.uint8).tolist() == [0xEE] * 33
    assert a.download(ptrs[2], (418,), np.uint8).tolist() == [k % 256 for k in range(418)]


def _one_byte(g, a, addr, value=0x00):
    g.poke(addr, value)
    with pytest.raises(GuardError) as e:
        a.check()
    return e.value


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_last_guard_byte_before_a_buffer(arena, k):
    g, a, ptrs = arena
    e = _one_byte(g, a, ptrs[k] - 1)
    assert (e.index, e.side, e.first, e.last, e.count) == (k, "before", -1, -1, 1)
    assert "buffer %d " % k in str(e) and "before" in str(e) and "[%d bytes]" % LENGTHS[k] in str(e)


@pytest.mark.parametrize("k", [0, 1, 2, 3, 5])
def test_first_byte_behind_a_buffer(arena, k):
    g, a, ptrs = arena
    e = _one_byte(g, a, ptrs[k] + LENGTHS[k], 0xA5)
    assert (e.index, e.side, e.first, e.last, e.count) == (k, "after", LENGTHS[k], LENGTHS[k], 1)
    assert "buffer %d " % k in str(e) and "after" in str(e)


def test_a_run_over_the_end_gives_first_and_last_offset(arena):
    g, a, ptrs = arena
    for d in range(15):                                            # a 16-byte store that began at the 33-byte row's last byte
        g.poke(ptrs[1] + 33 + d, 0xFF)
    with pytest.raises(GuardError) as e:
        a.check()
    assert (e.value.index, e.value.side, e.value.first, e.value.last, e.value.count) == (1, "after", 33, 47, 15)


def test_first_byte_of_the_arena_and_last_byte_of_the_tail_guard(arena):
    g, a, ptrs = arena
    e = _one_byte(g, a, a.base + a.capacity - 1)
    last = len(LENGTHS) - 1
    assert (e.index, e.side) == (last, "after") and e.first == e.last == a.base + a.capacity - 1 - ptrs[last]
    g.poke(a.base + a.capacity - 1, GUARD)
    e = _one_byte(g, a, a.base)
    assert (e.index, e.side, e.first) == (0, "before", a.base - ptrs[0])


@pytest.mark.parametrize("k,at", [(0, 0), (2, 417), (2, 200), (6, 33 * 65 + 31)])
def test_one_byte_of_a_marked_input(arena, k, at):
    g, a, ptrs = arena
    a.mark_input(ptrs[k])
    a.check()
    e = _one_byte(g, a, ptrs[k] + at, (at + 1) % 256)
    assert (e.index, e.side, e.first, e.last, e.count) == (k, "input", at, at, 1)
    assert "buffer %d " % k in str(e) and "input" in str(e)


def test_the_guard_value_written_into_a_marked_input_is_reported(arena):
    g, a, ptrs = arena
    assert LENGTHS[2] > GUARD + 1
    a.mark_inputs(exclude=[ptrs[1], ptrs[3]])
    at = 7                                                         # the input holds 7 there, not the guard value
    e = _one_byte(g, a, ptrs[2] + at, GUARD)
    assert (e.index, e.side, e.first) == (2, "input", at)          # compared with the uploaded bytes, not with the pattern


def test_an_unmarked_buffer_may_change_and_a_later_upload_is_the_new_reference(arena):
    g, a, ptrs = arena
    g.poke(ptrs[2] + 5, 0xEE)
    a.check()                                                      # not marked: an output
    a.upload(ptrs[2], np.full(418, 9, dtype=np.uint8))
    a.mark_input(ptrs[2])
    a.check()
    with pytest.raises(AssertionError):
        a.upload(ptrs[1], np.zeros(34, dtype=np.uint8))            # the arena's own upload stays inside the buffer
    with pytest.raises(KeyError):
        a.mark_input(ptrs[1] + 33)
