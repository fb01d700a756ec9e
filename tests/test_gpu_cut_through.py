"""bppp_rp_cut_through{,_device} against rangeproof.cut_through_host (tests/test_cut_through_host.py checks the restatement itself): every output
compared exactly — the new pool byte for byte, the one sum's entries, row_map, out_rows, every entry's verdict, the summed claim and the counts.
Rows are byte strings (tests/cut_through_jobs.py): the call never lifts a point.  Each case first checks what the call ran (table slots, groups,
sort passes: bppp_test_rp_cut_through_last).  The hook bppp_test_rp_cut_through_force reaches the collision and probe paths at small sizes: every
hash equal and the smallest table; and two pinned salts must give equal outputs."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from cut_through_jobs import N, hand_made, hand_made_two_ranges, one_identity, random_job, widen
from rp_backends import OracleBackend
from test_rangeproof import EXAMPLES

pytestmark = pytest.mark.gpu

ERR_ARG = -1
TWO = {"basisSeed": "test points", "argument": "IP", "ranges": [{"base": 16, "min": 0, "max": 2**64, "isOutput": True, "count": 2}]}
SALTS = (bytes(range(16)), bytes(range(100, 116)))
SIZES = [1, 63, 64, 65, 255, 256, 257, 2**14]
_HOST = {}


@pytest.fixture(scope="module")
def handles(gpu, oracle_lib):
    made = {}

    def get(name):
        if name not in made:
            schema = TWO if name == "two" else json.load(open(os.path.join(EXAMPLES, name, "schema.json")))
            st = (BRP if schema.get("binary") else RP).setup_from_schema(OracleBackend(oracle_lib), schema)
            made[name] = (BRP.NativeBinaryRangeProofs if schema.get("binary") else RP.NativeRangeProofs)(gpu, st)
        return made[name]
    yield get
    tl = capi.load_test_library()
    for nat in made.values():
        tl.bppp_test_rp_cut_through_force(nat.h, 0, None, 0)
        nat.close()


def _binary(nat):
    return isinstance(nat, BRP.NativeBinaryRangeProofs)


def _claims(nat, j):
    c = j["claims"]
    return c if c is None or not _binary(nat) else [(a, o) for a, _, o in c]


def _want(nat, key, j):
    """the restatement's answer, computed once per (handle kind, job)"""
    k = (_binary(nat), key)
    if k not in _HOST:
        _HOST[k] = RP.cut_through_host(j["nranges"], j["rows"], j["sum_start"], j["entries"], _claims(nat, j))
    return _HOST[k]


def _force(nat, mode=0, salt=None, bits=0):
    buf = (C.c_uint8 * 16)(*salt) if salt is not None else None
    assert capi.load_test_library().bppp_test_rp_cut_through_force(nat.h, mode, buf, bits) == 0


def _run(nat, j, device, alloc=None):
    """alloc: another allocator than the handle's context (tests/guard_arena.py); the two outputs then have their documented capacities to the byte"""
    cl = _claims(nat, j)
    if not device:
        return nat.cut_through(j["rows"], j["sum_start"], j["entries"], cl)
    g, cb, least = alloc or nat.gpu, nat.shape["coms_bytes"], 0 if alloc else 16
    rows, nnz = len(j["rows"]), len(j["entries"])
    ss, en, nsums, _ = nat._tally_csr(j["sum_start"], j["entries"])
    amt, typ, off = nat._tally_claim_arrays(cl, nsums)
    d = [g.to_device(np.frombuffer(b"".join(j["rows"]) or b"\0", dtype=np.uint8)), g.to_device(ss), g.to_device(en)]
    d += [g.to_device(a) if cl is not None and not (a is typ and _binary(nat)) else 0 for a in (amt, typ, off)]
    d += [g.alloc(max(rows * cb, least)), g.alloc(max(nnz * 4, least))]
    try:
        r = nat.cut_through_device(rows, d[0], nsums, d[1], d[2], nnz, d[3], d[4], d[5], d[6], d[7])
        nr_, nn = r.counts["new_rows"], r.counts["new_nnz"]
        pool = g.download(d[6], (max(nr_ * cb, 1),), dtype=np.uint8)
        r.coms_files = [pool[k * cb:(k + 1) * cb].tobytes() for k in range(nr_)]
        r.entries = [int(v) for v in g.download(d[7], (max(nn, 1),), dtype=np.uint32)[:nn]]
        return r
    finally:
        for p in d:
            if p:
                g.free(p)


def _same(got, want):
    assert got.counts == want.counts
    assert got.row_map == want.row_map and got.out_rows == want.out_rows
    assert got.entry_status == want.entry_status
    assert got.entries == want.entries
    assert got.coms_files == want.coms_files
    assert got.claims == want.claims


def _geometry(nat, j, want, forced_bits=0):
    slots, groups, passes = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert capi.load_test_library().bppp_test_rp_cut_through_last(nat.h, C.byref(slots), C.byref(groups), C.byref(passes)) == 0
    nnz, nr = len(j["entries"]), j["nranges"]
    ids = {RP.cut_identity(nr, j["rows"][(e & 0x7FFFFFFF) // nr], (e & 0x7FFFFFFF) % nr) for e in j["entries"]}
    assert groups.value == len(ids)
    assert passes.value == max(1, -(-(2 * len(ids) - 1).bit_length() // 8))
    s = slots.value
    assert s & (s - 1) == 0 and s >= nnz
    if forced_bits:
        assert s == max(1 << forced_bits, 1 << (nnz - 1).bit_length())
    else:
        assert 2 * nnz <= s < 4 * nnz or (nnz == 1 and s == 2)


def _check(nat, key, j, device, mode=0, salt=None, bits=0):
    want = _want(nat, key, j)
    _force(nat, mode, salt, bits)
    try:
        got = _run(nat, j, device)
    finally:
        _force(nat)
    _geometry(nat, j, want, bits)
    _same(got, want)
    return got


HAND = {**hand_made(), **{"two:" + k: v for k, v in hand_made_two_ranges().items()}}


def _on(handles, name, j):
    """the handle a hand-made job runs on, and the job in that handle's row shape"""
    if j["nranges"] == 2:
        return handles("two"), j
    if name == "bin_test":
        return handles("bin_test"), widen(j, 3)
    return handles("64bit"), j


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("handle", ["64bit", "bin_test"])
def test_hand_made_jobs(handles, handle, device):
    for key, j in HAND.items():
        if j["nranges"] == 2 and handle != "64bit":
            continue                                        # the two-range jobs run once, on the two-range handle
        nat, jj = _on(handles, handle, j)
        _check(nat, (handle, key), jj, device)
        _check(nat, (handle, key), jj, device, mode=1, salt=SALTS[0], bits=1)
        a = _check(nat, (handle, key), jj, device, salt=SALTS[0])
        b = _check(nat, (handle, key), jj, device, salt=SALTS[1])
        _same(a, b)


@pytest.mark.parametrize("nnz", SIZES)
def test_random_jobs(handles, nnz):
    """about 30 % of the outputs spent inside the set, some identities up to 5 times on either side, x and x + p mixed, spends before outputs"""
    nat = handles("64bit")
    j = random_job(1000 + nnz, nnz)
    assert len(j["entries"]) == nnz
    want = _want(nat, ("rnd", nnz), j)
    if nnz >= 255:
        assert want.counts["ncut"] > nnz // 8 and want.counts["nagain"] > 0 and want.counts["new_nnz"] > nnz // 8
    for device in (False, True):
        _check(nat, ("rnd", nnz), j, device)
    a = _check(nat, ("rnd", nnz), j, True, salt=SALTS[0])
    b = _check(nat, ("rnd", nnz), j, False, salt=SALTS[1])
    _same(a, b)
    if nnz <= 300:
        for device in (False, True):
            _check(nat, ("rnd", nnz), j, device, mode=1, salt=SALTS[1], bits=1)


@pytest.mark.parametrize("nnz", [65, 257])
def test_random_jobs_two_ranges_and_binary(handles, nnz):
    j2 = random_job(2000 + nnz, nnz, nranges=2)
    for device in (False, True):
        _check(handles("two"), ("rnd2", nnz), j2, device)
        _check(handles("two"), ("rnd2", nnz), j2, device, mode=1, salt=SALTS[0], bits=1)
    j3 = widen(random_job(3000 + nnz, nnz), 3)
    for device in (False, True):
        _check(handles("bin_test"), ("rnd3", nnz), j3, device)


@pytest.mark.parametrize("alternate", [True, False], ids=["alternating", "all_added"])
def test_one_identity_many_times(handles, alternate):
    """2^16 entries of ONE identity: one slot, one group, one comparison an entry; alternating signs cancel to nothing, all added leave one KEPT and
    the rest KEPT_AGAIN"""
    nat, nnz = handles("64bit"), 2**16
    j = one_identity(nnz, alternate)
    got = _check(nat, ("one", alternate), j, True)
    assert got.counts == (dict(new_rows=0, out_rows=0, new_nnz=0, ncut=nnz, nagain=0) if alternate else dict(new_rows=2, out_rows=2, new_nnz=nnz, ncut=0, nagain=nnz - 1))
    small = one_identity(300, alternate)
    _check(nat, ("one300", alternate), small, False, mode=1, salt=SALTS[0], bits=1)


def test_empty_jobs(handles):
    nat = handles("64bit")
    j = hand_made()["chain"]
    for device in (False, True):
        for jj in (dict(j, sum_start=[0], entries=[], claims=None), dict(j, sum_start=[0, 0, 0], entries=[], claims=[(1, 2, 3), (4, 5, 6)])):
            got = _run(nat, jj, device)
            want = RP.cut_through_host(1, jj["rows"], jj["sum_start"], jj["entries"], jj["claims"])
            _same(got, want)
            assert got.counts == dict(new_rows=0, out_rows=0, new_nnz=0, ncut=0, nagain=0)


class _Raw:
    """one call through the C ABI with every output buffer pre-filled with a pattern"""
    PAT = 0xA5

    def __init__(self, nat, j, device, amt="job", typ="job", off="job", want_claims=True):
        self.nat, self.device, g = nat, device, nat.gpu
        cb = nat.shape["coms_bytes"]
        self.rows, self.nnz = len(j["rows"]), len(j["entries"])
        ss, en, self.nsums, _ = nat._tally_csr(j["sum_start"], j["entries"])
        a, t, o = nat._tally_claim_arrays(_claims(nat, j), self.nsums)
        pick = lambda arg, arr: arr if isinstance(arg, str) else arg
        self.host_in = [np.frombuffer(b"".join(j["rows"]), dtype=np.uint8), ss, en, pick(amt, a), pick(typ, t), pick(off, o)]
        self.status, self.row_map = np.full(self.nnz, 0xA5A5A5A5, dtype=np.uint32), np.full(self.rows, 0xA5A5A5A5, dtype=np.uint32)
        self.new_coms, self.new_entries = np.full(self.rows * cb, self.PAT, dtype=np.uint8), np.full(self.nnz, 0xA5A5A5A5, dtype=np.uint32)
        self.claims = np.full((3, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64) if want_claims else None
        self.counts = capi.RpCutCounts(*[0xA5] * 5)
        self.dev = []
        if device:
            self.dev = [g.to_device(x) if x is not None else 0 for x in self.host_in] + [g.to_device(self.new_coms), g.to_device(self.new_entries)]

    def call(self):
        vp = lambda x: C.c_void_p(x.ctypes.data) if x is not None else None
        lib = self.nat.gpu.lib
        if self.device:
            p = [C.c_void_p(x) for x in self.dev]
            return lib.bppp_rp_cut_through_device(self.nat.h, self.rows, p[0], self.nsums, p[1], p[2], self.nnz, p[3], p[4], p[5], vp(self.status), vp(self.row_map), p[6], p[7],
                                                  vp(self.claims), C.byref(self.counts))
        i = self.host_in
        return lib.bppp_rp_cut_through(self.nat.h, self.rows, vp(i[0]), self.nsums, vp(i[1]), vp(i[2]), self.nnz, vp(i[3]), vp(i[4]), vp(i[5]), vp(self.status), vp(self.row_map),
                                       vp(self.new_coms), vp(self.new_entries), vp(self.claims), C.byref(self.counts))

    def untouched(self):
        g = self.nat.gpu
        if self.device:
            self.new_coms = g.download(self.dev[6], self.new_coms.shape, dtype=np.uint8)
            self.new_entries = g.download(self.dev[7], self.new_entries.shape, dtype=np.uint32)
        return (np.all(self.status == 0xA5A5A5A5) and np.all(self.row_map == 0xA5A5A5A5) and np.all(self.new_coms == self.PAT) and np.all(self.new_entries == 0xA5A5A5A5)
                and (self.claims is None or np.all(self.claims == 0xA5A5A5A5A5A5A5A5)) and all(getattr(self.counts, n) == 0xA5 for n, _ in capi.RpCutCounts._fields_))

    def close(self):
        for p in self.dev:
            if p:
                self.nat.gpu.free(p)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_documented_errors_leave_the_outputs_untouched(handles, gpu, device):
    nat = handles("64bit")
    base = hand_made()["claims"]                             # 4 rows, 2 sums, 4 entries, claims
    err = lambda: gpu.lib.bppp_last_error(gpu.h).decode()
    amt_only = nat._tally_claim_arrays(base["claims"], 2)[0]
    cases = [
        (dict(base, sum_start=[0, 3, 2]), {}, "rp_cut_through: sum_start[2] = 2 is not non-decreasing from 0 to nnz = 4"),
        (dict(base, sum_start=[1, 2, 4]), {}, "rp_cut_through: sum_start[0] = 1"),
        (dict(base, entries=base["entries"][:3] + [RP.tally_entry(4, True)]), {}, "rp_cut_through: entries[3]: index 4 is not below rows * nranges = 4"),
        (base, dict(amt=amt_only, typ=None, off=None), "rp_cut_through: claim_amounts, claim_types and claim_offsets must be given together or all be NULL"),
        (dict(base, claims=[(1, 2, 3), (4, N, 5)]), {}, "rp_cut_through: sum 1: a claimed type or offset is not canonical (>= n)"),
        (dict(base, claims=[(1, 2, N + 1), (4, 0, N)]), {}, "rp_cut_through: sum 0: a claimed type or offset is not canonical (>= n)"),
        (base, dict(want_claims=False), "rp_cut_through: null input"),
    ]
    for j, kw, text in cases:
        raw = _Raw(nat, j, device, **kw)
        try:
            assert raw.call() == ERR_ARG, text
            assert err().startswith(text), (err(), text)
            assert raw.untouched(), text
        finally:
            raw.close()
    # and the same buffers with a good job are all written
    raw = _Raw(nat, base, device)
    try:
        assert raw.call() == 0 and not raw.untouched() and raw.counts.new_nnz == 2 and raw.counts.ncut == 2
    finally:
        raw.close()


def test_nothing_rests_on_leftovers(handles, gpu):
    """after both poison hooks with 0x00 and 0xFF, and after a larger job followed by a smaller one, the outputs are unchanged"""
    nat, tl = handles("64bit"), capi.load_test_library()
    big, small = random_job(77, 3000), random_job(78, 257)
    want_small = _want(nat, ("left", 257), small)
    _check(nat, ("left", 3000), big, True)
    _check(nat, ("left", 257), small, True)
    for byte in (0x00, 0xFF):
        n = C.c_uint64()
        assert tl.bppp_test_rp_poison(nat.h, byte, C.byref(n)) == 0 and n.value > 0
        assert tl.bppp_test_ctx_poison(gpu.h, byte, C.byref(n)) == 0
        for device in (True, False):
            _same(_run(nat, small, device), want_small)
        assert tl.bppp_test_rp_poison(nat.h, byte, C.byref(n)) == 0
        _check(nat, ("left", 257), small, True, mode=1, salt=SALTS[0], bits=1)
