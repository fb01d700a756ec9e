"""The set commitments (bppp_rp_set_*) against the hashlib restatement of rangeproof.py (tests/test_set_host.py checks the restatement itself against
a naive recursive definition): roots, peaks and paths byte for byte, verdicts one by one.  Every library call runs directly after
bppp_test_rp_poison has filled the handle's workspaces, and every host output buffer - roots, peaks, paths, the four words of info, the statuses and
the accept word - is handed to the C ABI at its documented size between sentinel bytes that must survive (Poisoned and verify below).  The
production wrappers of rangeproof.py are called next to them and must answer the same.  Rows are slices of one seeded blob, and the restatement's
states are computed once and shared."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import bulletproofspp_amd as b
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from rp_backends import OracleBackend
from test_rangeproof import EXAMPLES

pytestmark = pytest.mark.gpu

TAG = b"set test"
NMAX = 65537 + 700
_BLOB = np.random.default_rng(20261021).integers(0, 256, size=max(NMAX * 33, 300 * 8192), dtype=np.uint8).tobytes()
_STATE = {}                                                     # (tag, n) -> peaks of the first n rows of 33 bytes
_LEVELS = {}


def rows33(lo, hi):
    return [_BLOB[33 * i:33 * i + 33] for i in range(lo, hi)]


def rows_of(rb, n):
    """n rows of rb bytes cut from the same blob"""
    return [_BLOB[rb * i:rb * i + rb] for i in range(n)]


def peaks_at(n, tag=TAG):
    """the restatement's peaks of the first n 33-byte rows, continued from the largest state below n that is already known"""
    if (tag, n) not in _STATE:
        below = max([k for t, k in _STATE if t == tag and k < n], default=0)
        _STATE[(tag, n)] = RP.set_peaks_host(tag, rows33(below, n), start=(below, _STATE[(tag, below)]) if below else None)
    return _STATE[(tag, n)]


def root_at(n, tag=TAG, rb=33):
    return RP.set_root_host(tag, rb, n, peaks_at(n, tag))


def levels_at(n):
    if n not in _LEVELS:
        _LEVELS[n] = RP.set_levels_host(TAG, rows33(0, n))
    return _LEVELS[n]


@pytest.fixture(scope="module")
def nat(gpu, oracle_lib):
    st = RP.setup_from_schema(OracleBackend(oracle_lib), json.load(open(os.path.join(EXAMPLES, "64bit", "schema.json"))))
    h = RP.NativeRangeProofs(gpu, st, oracle_tag=TAG)
    yield h
    h.close()


def poison(nat, byte=0xEE):
    n = C.c_uint64(0)
    assert capi.load_test_library().bppp_test_rp_poison(nat.h, byte, C.byref(n)) == 0


GUARD = 64


def guarded(nbytes):
    """a host output buffer of nbytes with GUARD sentinel bytes in front of it and behind it"""
    return np.full(nbytes + 2 * GUARD, 0xA5, dtype=np.uint8)


def at(buf, offset=0, ctype=None):
    addr = buf.ctypes.data + GUARD + offset
    return C.c_void_p(addr) if ctype is None else C.cast(C.c_void_p(addr), C.POINTER(ctype))


def unguard(buf, nbytes):
    assert len(buf) == nbytes + 2 * GUARD and buf[:GUARD].tobytes() == b"\xa5" * GUARD == buf[GUARD + nbytes:].tobytes(), "the call wrote outside its output buffer"
    return buf[GUARD:GUARD + nbytes].tobytes()


class Poisoned:
    """A CommitmentSet driven through the C ABI itself: every call runs directly after the poison hook and writes into a buffer of exactly the
    documented size between sentinels.  `cs` is the production wrapper, whose own answers same_state compares with these."""

    def __init__(self, nat, cs):
        self.nat, self.cs, self.lib = nat, cs, nat.gpu.lib

    def _call(self, name, byte, *args):
        poison(self.nat, byte)
        self.nat.gpu._check(getattr(self.lib, name)(self.cs.h, *args), name)

    def append(self, rows):
        poison(self.nat, 0xEE)
        self.cs.append(rows)

    def close(self):
        self.cs.close()

    def info(self):
        buf = guarded(32)
        self._call("bppp_rp_set_info", 0x5C, at(buf, 0, C.c_uint64), at(buf, 8, C.c_size_t), at(buf, 16, C.c_size_t), at(buf, 24, C.c_size_t))
        return dict(zip(("n", "row_bytes", "npeaks", "store_bytes"), (int(v) for v in np.frombuffer(unguard(buf, 32), dtype=np.uint64))))

    def root(self):
        buf = guarded(32)
        self._call("bppp_rp_set_root", 0x5C, at(buf))
        return unguard(buf, 32)

    def peaks(self):
        m = bin(self.cs.info()["n"]).count("1")
        buf = guarded(32 * m)
        self._call("bppp_rp_set_peaks", 0x5C, at(buf))
        out = unguard(buf, 32 * m)
        return [out[32 * p:32 * p + 32] for p in range(m)]

    def paths(self, idx):
        pb, nq = RP.set_path_bytes(self.cs.info()["n"]), len(idx)
        ix = np.array(list(idx) or [0], dtype=np.uint64)
        buf = guarded(nq * pb)
        self._call("bppp_rp_set_paths", 0x5C, nq, C.c_void_p(ix.ctypes.data), at(buf))
        out = unguard(buf, nq * pb)
        return [out[pb * q:pb * q + pb] for q in range(nq)]


def verify(nat, rb, n, root, idx, rows, paths, want_status=True):
    """bppp_rp_set_verify_paths after the poison hook, status and accept between sentinels: (accept, statuses) or accept"""
    nq, pb = len(idx), RP.set_path_bytes(n)
    ix = np.array([int(i) % 2**64 for i in idx] or [0], dtype=np.uint64)
    rw, pt, rt = (np.frombuffer(x or b"\0", dtype=np.uint8) for x in (b"".join(rows), b"".join(paths), bytes(root)))
    st, acc = guarded(4 * nq), guarded(4)
    poison(nat)
    rc = nat.gpu.lib.bppp_rp_set_verify_paths(nat.h, rb, n, C.c_void_p(rt.ctypes.data), nq, C.c_void_p(ix.ctypes.data), C.c_void_p(rw.ctypes.data),
                                              C.c_void_p(pt.ctypes.data) if pb else None, at(st) if want_status else None, at(acc, 0, C.c_int))
    nat.gpu._check(rc, "bppp_rp_set_verify_paths")
    accept = int(np.frombuffer(unguard(acc, 4), dtype=np.int32)[0])
    assert accept in (0, 1)
    status = [int(v) for v in np.frombuffer(unguard(st, 4 * nq), dtype=np.uint32)]
    return (bool(accept), status) if want_status else bool(accept)


def make(nat, rb=33, keep=True):
    return Poisoned(nat, nat.commitment_set(rb, keep))


def same_state(cs, n, tag=TAG):
    assert cs.root() == root_at(n, tag) == cs.cs.root()
    assert cs.peaks() == peaks_at(n, tag) == cs.cs.peaks()
    info = cs.info()
    assert info == cs.cs.info()
    assert (info["n"], info["row_bytes"], info["npeaks"]) == (n, 33, bin(n).count("1"))
    assert info["store_bytes"] >= (64 * n - 32 * info["npeaks"] if cs.cs.keep_nodes else 2048)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537])
def test_roots_and_peaks(nat, n):
    for keep in (True, False):
        cs = make(nat, 33, keep)
        cs.append(rows33(0, n))
        same_state(cs, n)
        cs.close()


@pytest.mark.parametrize("n0", [0, 1, 255, 256, 257, 65535])
@pytest.mark.parametrize("m", [0, 1, 2, 255, 256, 257, 700])
def test_append_onto(nat, n0, m):
    sets = [make(nat, 33, True), make(nat, 33, False)]
    for cs in sets:
        cs.append(rows33(0, n0))
        assert cs.root() == root_at(n0)
    sets.append(Poisoned(nat, RP.CommitmentSet.restore(nat, 33, n0, sets[1].peaks())))
    for cs in sets:
        cs.append(b"".join(rows33(n0, n0 + m)))
        same_state(cs, n0 + m)
        cs.close()


def test_a_chain_of_appends(nat):
    rnd = random.Random(5)
    sets, n = [make(nat, 33, True), make(nat, 33, False)], 0
    for step in range(40):
        m = rnd.randrange(601)
        if step == 20:
            sets.append(Poisoned(nat, RP.CommitmentSet.restore(nat, 33, n, sets[1].peaks())))
        for cs in sets:
            cs.append(rows33(n, n + m))
        n += m
        want = root_at(n)
        assert [cs.root() for cs in sets] == [want] * len(sets), (step, n, m)
    for cs in sets:
        same_state(cs, n)
        cs.close()


@pytest.mark.parametrize("rb", [1, 23, 24, 33, 87, 88, 2056, 8192])
def test_row_lengths(nat, rb):
    n = 300
    rows = rows_of(rb, n)
    levels = RP.set_levels_host(TAG, rows)
    peaks = RP.set_peaks_host(TAG, rows)
    root = RP.set_root_host(TAG, rb, n, peaks)
    full, front = make(nat, rb, True), make(nat, rb, False)
    for cs in (full, front):
        cs.append(rows[:129])
        cs.append(rows[129:])
        assert cs.root() == root and cs.peaks() == peaks
    idx = [0, 1, 128, 255, 256, 287, 288, 299]
    paths = full.paths(idx)
    assert paths == [RP.set_path_host(TAG, rows, i, levels) for i in idx]
    assert verify(nat, rb, n, root, idx, [rows[i] for i in idx], paths) == (True, [0] * len(idx))
    assert full.cs.paths(idx) == paths and nat.set_verify_paths(rb, n, root, idx, [rows[i] for i in idx], paths, want_status=True) == (True, [0] * len(idx))
    bad = [bytes([rows[i][0] ^ 1]) + rows[i][1:] for i in idx[:-1]] + [rows[idx[-1]][:-1] + bytes([rows[idx[-1]][-1] ^ 0x80])]
    assert verify(nat, rb, n, root, idx, bad, paths) == (False, [RP.SET_MISMATCH] * len(idx))
    assert nat.set_verify_paths(rb, n, root, idx, bad, paths) is False
    full.close()
    front.close()


def flip(bs, o, bit=1):
    return bs[:o] + bytes([bs[o] ^ bit]) + bs[o + 1:]


def single_changes(rnd, n, i, row, path):
    """queries that differ from the honest one (i, row, path) in one place, under the honest n and root"""
    h, p, m = RP._set_locate(n, i)
    used = 32 * (h + p + (1 if p < m - 1 else 0))
    out = [(i, flip(row, rnd.randrange(len(row)), 1 << rnd.randrange(8)), path)]
    if used:
        out += [(i, row, flip(path, o)) for o in (0, used - 1, rnd.randrange(used))]
    if used < len(path):
        out += [(i, row, flip(path, o, 0x40)) for o in (used, len(path) - 1)]
    out += [(j, row, path) for j in {(i + 1) % n, i ^ 1, n - 1 - i, n, n + 1, 2**63, 2**64 - 1} if j != i]
    return out


def judge(nat, n, root, queries, rb=33):
    """the library's verdicts on the queries equal the restatement's, and accept follows"""
    want = [RP.set_verify_path_host(TAG, rb, n, root, i, r, p) for i, r, p in queries]
    got = verify(nat, rb, n, root, [q[0] for q in queries], [q[1] for q in queries], [q[2] for q in queries])
    assert got == (all(w == RP.SET_OK for w in want), want)
    assert verify(nat, rb, n, root, [q[0] for q in queries], [q[1] for q in queries], [q[2] for q in queries], want_status=False) == got[0]
    return want


def other_n_and_root(nat, rnd, n, root, honest):
    """the honest queries under a changed n (the paths cut or zero-padded where the length changes) and under a changed root"""
    for n2 in {n - 1, n + 1, n ^ 2, 2 * n, n + 2**40} - {n, 0}:
        pb = RP.set_path_bytes(n2)
        judge(nat, n2, root, [(i, r, p[:pb].ljust(pb, b"\0")) for i, r, p in honest])
    assert set(judge(nat, n, flip(root, rnd.randrange(32), 1 << rnd.randrange(8)), honest)) == {RP.SET_MISMATCH}


@pytest.mark.parametrize("n", [1, 2, 3, 77, 256, 600])
def test_every_path(nat, n):
    rnd = random.Random(n)
    rows, levels, root = rows33(0, n), levels_at(n), root_at(n)
    cs = make(nat, 33, True)
    cs.append(rows[:n // 3])
    cs.append(rows[n // 3:])
    paths = cs.paths(list(range(n)))
    assert paths == [RP.set_path_host(TAG, rows, i, levels) for i in range(n)]
    honest = [(i, rows[i], paths[i]) for i in range(n)]
    assert set(judge(nat, n, root, honest)) == {RP.SET_OK}
    changed = [q for i in sorted({0, n - 1, n // 2, rnd.randrange(n), rnd.randrange(n)}) for q in single_changes(rnd, n, i, rows[i], paths[i])]
    want = judge(nat, n, root, honest[:3] + changed)
    assert RP.SET_MISMATCH in want and RP.SET_BAD_INDEX in want and (n < 3 or RP.SET_BAD_PADDING in want)
    other_n_and_root(nat, rnd, n, root, honest[:40])
    cs.close()


def test_paths_behind_the_second_tile_level(nat):
    n, idx = 65537, [0, 1, 255, 256, 65535, 65536]
    rnd = random.Random(1)
    rows, levels, root = rows33(0, n), levels_at(n), root_at(n)
    cs = make(nat, 33, True)
    cs.append(rows[:65535])
    cs.append(rows[65535:])
    paths = cs.paths(idx)
    assert paths == [RP.set_path_host(TAG, rows, i, levels) for i in idx]
    honest = [(i, rows[i], p) for i, p in zip(idx, paths)]
    assert set(judge(nat, n, root, honest)) == {RP.SET_OK}
    judge(nat, n, root, [q for i, r, p in honest for q in single_changes(rnd, n, i, r, p)])
    other_n_and_root(nat, rnd, n, root, honest)
    cs.close()


def test_verify_against_the_empty_set(nat):
    """n = 0: a path has no bytes (paths may be NULL), every index is BAD_INDEX, and no query at all is accepted"""
    root = RP.set_root_host(TAG, 33, 0, [])
    cs = make(nat, 33, False)
    assert cs.root() == root and cs.peaks() == [] and RP.set_path_bytes(0) == 0
    cs.close()
    rows = rows33(0, 3)
    judge(nat, 0, root, [(0, rows[0], b""), (5, rows[1], b""), (2**64 - 1, rows[2], b"")])
    assert verify(nat, 33, 0, root, [0, 5, 2**64 - 1], rows, [b""] * 3) == (False, [RP.SET_BAD_INDEX] * 3)
    assert nat.set_verify_paths(33, 0, root, [0], rows[:1], [b""], want_status=True) == (False, [RP.SET_BAD_INDEX])
    assert verify(nat, 33, 0, root, [], [], []) == (True, []) and verify(nat, 33, 600, root_at(600), [], [], []) == (True, [])
    judge(nat, 0, root_at(1), [(0, rows[0], b"")])            # the root of another set changes nothing: the index is judged first


def test_refusals(nat, gpu):
    lib, n = gpu.lib, 300
    full, front = make(nat, 33, True), make(nat, 33, False)
    for cs in (full, front):
        cs.append(rows33(0, n))
    with pytest.raises(b.BpppError, match="frontier alone"):
        front.paths([0])
    # an index at or above n: the first one is named and nothing is written
    idx = np.array([5, 299, 300, 7, 400], dtype=np.uint64)
    out = np.full(5 * RP.set_path_bytes(n) + 64, 0xA5, dtype=np.uint8)
    poison(nat)
    assert lib.bppp_rp_set_paths(full.cs.h, 5, C.c_void_p(idx.ctypes.data), C.c_void_p(out.ctypes.data)) == -1
    assert b"idx[2] = 300" in lib.bppp_last_error(gpu.h) and bytes(out) == b"\xa5" * len(out)
    # refused appends leave the set as it was: too many rows for the store, for one call, and no rows at all
    one = np.zeros(33, dtype=np.uint8)
    for cs, nrows, text in ((full, 2**31 - 300, b"a full store holds fewer than 2^31"), (front, 2**31, b"is 2^31 or more"), (full, 2**31, b"is 2^31 or more")):
        before = (cs.root(), cs.info())
        poison(nat)
        assert lib.bppp_rp_set_append(cs.cs.h, nrows, C.c_void_p(one.ctypes.data)) == -1 and text in lib.bppp_last_error(gpu.h)
        assert lib.bppp_rp_set_append(cs.cs.h, 1, None) == -1 and b"rows is NULL" in lib.bppp_last_error(gpu.h)
        assert (cs.root(), cs.info()) == before == (root_at(n), before[1])
    stated = [bytes([k]) * 32 for k in range(62)]
    far = Poisoned(nat, RP.CommitmentSet.restore(nat, 33, 2**63 - 2, stated))
    assert far.root() == RP.set_root_host(TAG, 33, 2**63 - 2, stated) and far.peaks() == stated
    far.append(rows33(0, 1))
    assert far.info()["n"] == 2**63 - 1
    assert far.root() == RP.set_root_host(TAG, 33, 2**63 - 1, RP.set_peaks_host(TAG, rows33(0, 1), start=(2**63 - 2, stated)))
    before = far.root()
    with pytest.raises(b.BpppError, match="fewer than 2\\^63"):
        far.append(rows33(0, 1))
    assert far.root() == before
    for cs in (full, front, far):
        cs.close()


def test_the_tag_separates_sets(nat, gpu):
    n = 257
    same = RP.NativeRangeProofs(gpu, nat.st, oracle_tag=TAG)
    other = RP.NativeRangeProofs(gpu, nat.st, oracle_tag=b"another chain")
    roots = []
    for h in (nat, same, other):
        cs = Poisoned(h, h.commitment_set(33, True))
        cs.append(rows33(0, n))
        roots.append(cs.root())
        if h is other:
            assert cs.root() == root_at(n, b"another chain") and cs.paths([256])[0] != RP.set_path_host(TAG, rows33(0, n), 256, levels_at(n))
        cs.close()
    assert roots[0] == roots[1] == root_at(n) and roots[2] != roots[0]
    same.close()
    other.close()
