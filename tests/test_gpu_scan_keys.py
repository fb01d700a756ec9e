"""bppp_rp_scan_keys{,_device}: an output set scanned under many view secrets in one call.  The specification is one sentence — for every key k and
row i, exactly what bppp_rp_scan with view_secrets[k] reports for row i — so the expectation is K calls of the existing scan (nat.scan, which
tests/test_gpu_seal_scan.py pins to rangeproof.scan_host) over that file's corpus of 257 rows per setup: owned rows, another account's rows, two
kinds of bad hint, three kinds of tag-only row and the engineered tag collision.  rangeproof.scan_keys_host itself is compared on the first 16 rows.

The key list is a, other, a again, then seeded random secrets that own nothing, 2 KT + 1 = 33 keys in all; the smaller key counts are its prefixes.
Under the 30 random keys about 30 * 193 / 256 = 22 rows match a tag by chance (none with probability e^-22), and the collision row is OWNED under
`other` and TAG_ONLY under `a`: the test asserts both before it relies on them."""
import ctypes as C
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from rp_backends import OracleBackend
from test_gpu_seal_scan import COLLISION_ROW, _Buffers, _bytes_array, _data, handles  # noqa: F401  (handles: the module's fixture of native handles)

pytestmark = pytest.mark.gpu

N = O.N
ERR_ARG = -1
NAMES = ["rec_test", "bin_test"]
COUNTS = (1, 2, 63, 64, 65, 257)
FOREIGN, OWNED, BAD_HINT, TAG_ONLY = RP.SCAN_FOREIGN, RP.SCAN_OWNED, RP.SCAN_BAD_HINT, RP.SCAN_TAG_ONLY
_EXPECT = {}


def _geometry(nat, rows, nkeys):
    out = np.zeros(3, dtype=np.uint64)
    assert capi.load_test_library().bppp_test_rp_scan_keys_geometry(nat.h, rows, nkeys, C.c_void_p(out.ctypes.data)) == 0
    return [int(v) for v in out]


def _last_error(nat):
    return nat.gpu.lib.bppp_last_error(nat.gpu.h).decode()


def _expect(oracle_lib, handles, name):
    """keys, and single[k] = (statuses, openings) of nat.scan under keys[k] over the whole corpus: computed once per setup"""
    if name not in _EXPECT:
        D, nat = _data(oracle_lib, name), handles(name)
        KT = _geometry(nat, 257, 2**20)[1]
        rng = random.Random("scan keys " + name)
        keys = [D["a"], D["other"], D["a"]] + [rng.randrange(1, N) for _ in range(2 * KT + 1 - 3)]
        single = [nat.scan(k, D["scan_files"], D["scan_seals"])[:2] for k in keys]
        _EXPECT[name] = (keys, single, KT)
    return _EXPECT[name]


def _want(single, nkeys, rows):
    """(row_status, hits, ntag_only) of the first nkeys keys over the first rows rows, from the K single scans"""
    hits = [(k, i, single[k][1][i]) for i in range(rows) for k in range(nkeys) if single[k][0][i] == OWNED]
    ntag = sum(single[k][0][i] == TAG_ONLY for i in range(rows) for k in range(nkeys))
    row_status = []
    for i in range(rows):
        col = [single[k][0][i] for k in range(nkeys)]
        row_status.append(next((v for v in (BAD_HINT, OWNED, TAG_ONLY) if v in col), FOREIGN))
    return row_status, hits, ntag


def _raw(nat, D, keys, rows, cap, device):
    """one call on 0xA5-filled outputs: (rc, row_status, hit_key [cap], hit_row [cap], openings [cap][nr], nhits, ntag_only)"""
    nr, lib, g = D["nr"], nat.gpu.lib, nat.gpu
    vp = lambda x: C.c_void_p(x.ctypes.data)
    sec = capi.scalars_to_array(list(keys))
    files, seals = _bytes_array(D["scan_files"][:rows] or [b"\0"]), _bytes_array(D["scan_seals"][:rows] or [b"\0"])
    status = np.full(max(rows, 1), 0xA5A5A5A5, dtype=np.uint32)
    hk, hr = np.full(max(cap, 1), 0xA5A5A5A5, dtype=np.uint32), np.full(max(cap, 1), 0xA5A5A5A5, dtype=np.uint32)
    nhits, ntag = C.c_size_t(12345), C.c_uint64(12345)
    if device:
        with _Buffers(g) as buf:
            outs = [buf.out(max(cap, 1) * nr * 32) for _ in range(3)]
            rc = lib.bppp_rp_scan_keys_device(nat.h, len(keys), vp(sec), rows, buf.up(files), buf.up(seals), vp(status), cap, vp(hk), vp(hr), *outs, C.byref(nhits), C.byref(ntag))
            v, t, bl = (capi.array_to_scalars(g.download(o, (max(cap, 1) * nr, 4), np.uint64)) for o in outs)
    else:
        outs = [np.full((max(cap, 1) * nr, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64) for _ in range(3)]
        rc = lib.bppp_rp_scan_keys(nat.h, len(keys), vp(sec), rows, vp(files), vp(seals), vp(status), cap, vp(hk), vp(hr), *(vp(o) for o in outs), C.byref(nhits), C.byref(ntag))
        v, t, bl = (capi.array_to_scalars(o) for o in outs)
    openings = [[(v[h * nr + i], t[h * nr + i], bl[h * nr + i]) for i in range(nr)] for h in range(cap)]
    return rc, [int(s) for s in status[:rows]], [int(x) for x in hk[:cap]], [int(x) for x in hr[:cap]], openings, int(nhits.value), int(ntag.value)


def _check(got, want, cap, nr):
    rc, row_status, hk, hr, openings, nhits, ntag = got
    want_status, want_hits, want_ntag = want
    assert rc == 0 and row_status == want_status and nhits == len(want_hits) and ntag == want_ntag
    n = min(nhits, cap)
    assert [(hk[h], hr[h], openings[h]) for h in range(n)] == want_hits[:n]                   # the first cap hits are the prefix of the full list
    assert hk[n:] == [0] * (cap - n) and hr[n:] == [0] * (cap - n) and openings[n:] == [[(0, 0, 0)] * nr] * (cap - n)


# ----------------------------------------------------------------------------- 1. the K single scans; host = device; every row and key count
@pytest.mark.parametrize("name", NAMES)
def test_scan_keys_equals_the_single_scans(gpu, oracle_lib, handles, name):
    D, nat = _data(oracle_lib, name), handles(name)
    keys, single, KT = _expect(oracle_lib, handles, name)
    nr, tl = D["nr"], capi.load_test_library()
    # what the corpus must hold for this test to mean something
    full = _want(single, len(keys), 257)
    assert any(single[k][0][i] == TAG_ONLY for k in range(3, len(keys)) for i in range(257)), "no chance tag match under the random keys: change the seed"
    assert single[0][0][COLLISION_ROW] == TAG_ONLY and single[1][0][COLLISION_ROW] == OWNED and full[0][COLLISION_ROW] == OWNED
    assert not any(single[k][0][i] == OWNED for k in range(3, len(keys)) for i in range(257)) and single[0] == single[2]
    assert {BAD_HINT, OWNED, TAG_ONLY} <= set(full[0])
    # rangeproof.scan_keys_host, the literal loop over the oracle backend, on the first 16 rows
    assert RP.scan_keys_host(OracleBackend(oracle_lib), D["st"], keys, D["scan_files"][:16], D["scan_seals"][:16]) == _want(single, len(keys), 16)
    poisoned = C.c_uint64(0)
    for rows in COUNTS:
        for nk in (1, 2, KT - 1, KT, KT + 1, 2 * KT + 1):
            want = _want(single, nk, rows)
            assert tl.bppp_test_rp_poison(nat.h, 0xEE, C.byref(poisoned)) == 0
            assert nat.scan_keys(keys[:nk], D["scan_files"][:rows], D["scan_seals"][:rows]) == want, (rows, nk)
            cap = len(want[1]) + 3
            _check(_raw(nat, D, keys[:nk], rows, cap, device=True), want, cap, nr)
    # the device wrapper: files and seals in HBM, the same three results (fewer hits than rows here: one call; the worst-case test below
    # needs the second)
    with _Buffers(nat.gpu) as buf:
        assert nat.scan_keys_device(keys, 257, buf.up(_bytes_array(D["scan_files"])), buf.up(_bytes_array(D["scan_seals"]))) == full
    # no output array at all: the verdicts and the counts alone
    vp = lambda x: C.c_void_p(x.ctypes.data)
    sec, nhits = capi.scalars_to_array(keys), C.c_size_t(0)
    files, seals = _bytes_array(D["scan_files"]), _bytes_array(D["scan_seals"])
    assert nat.gpu.lib.bppp_rp_scan_keys(nat.h, len(keys), vp(sec), 257, vp(files), vp(seals), None, 0, None, None, None, None, None, C.byref(nhits), None) == 0
    assert nhits.value == len(full[1])


# ----------------------------------------------------------------------------- 2. several row passes, key tiles and open chunks, over poison
@pytest.mark.parametrize("name", NAMES)
def test_scan_keys_in_passes_tiles_and_chunks(gpu, oracle_lib, handles, name):
    D, nat = _data(oracle_lib, name), handles(name)
    keys, single, KT = _expect(oracle_lib, handles, name)
    nr, tl = D["nr"], capi.load_test_library()
    poisoned = C.c_uint64(0)
    try:
        assert tl.bppp_test_rp_set_flat_chunk(nat.h, nr * 16 * 64) == 0
        rows_pass, kt, chunk = _geometry(nat, 257, len(keys))
        assert 3 * rows_pass <= 257 and 2 * kt <= len(keys)                                      # at least three row passes and two key tiles
        survivors = sum(single[k][0][i] in (OWNED, TAG_ONLY) for k in range(kt) for i in range(rows_pass))
        assert survivors > chunk                                                                 # the first tile of the first pass opens in two chunks at least
        for rows in (65, 257):
            want = _want(single, len(keys), rows)
            assert tl.bppp_test_rp_poison(nat.h, 0x5C, C.byref(poisoned)) == 0 and poisoned.value > 0
            assert nat.scan_keys(keys, D["scan_files"][:rows], D["scan_seals"][:rows]) == want, rows
            cap = len(want[1])
            _check(_raw(nat, D, keys, rows, cap, device=True), want, cap, nr)
    finally:
        assert tl.bppp_test_rp_set_flat_chunk(nat.h, 0) == 0


# ----------------------------------------------------------------------------- 3. cap below, at and above the hit count
@pytest.mark.parametrize("name", NAMES)
def test_scan_keys_cap(gpu, oracle_lib, handles, name):
    D, nat = _data(oracle_lib, name), handles(name)
    keys, single, KT = _expect(oracle_lib, handles, name)
    rows, nk = 65, KT + 1
    want = _want(single, nk, rows)
    nhits = len(want[1])
    assert nhits > 3
    for cap in (0, 1, nhits - 1, nhits, nhits + 3):
        for device in (False, True):
            _check(_raw(nat, D, keys[:nk], rows, cap, device), want, cap, D["nr"])


# ----------------------------------------------------------------------------- 4. the worst case: every pair a survivor, every pair owned
@pytest.mark.parametrize("name", NAMES)
def test_scan_keys_when_every_pair_is_owned(gpu, oracle_lib, handles, name):
    D, nat = _data(oracle_lib, name), handles(name)
    keys, single, KT = _expect(oracle_lib, handles, name)
    tl, nr = capi.load_test_library(), D["nr"]
    mine = [b for b in range(257) if b % 8 in (0, 2)]
    assert len(mine) == 65 and all(single[0][0][b] == OWNED for b in mine)
    files, seals = [D["scan_files"][b] for b in mine], [D["scan_seals"][b] for b in mine]
    try:
        assert tl.bppp_test_rp_set_flat_chunk(nat.h, nr * 16 * 64) == 0
        kt = _geometry(nat, 65, KT + 1)[1]
        assert kt == KT
        status, hits, ntag = nat.scan_keys([D["a"]] * (KT + 1), files, seals)
        assert status == [OWNED] * 65 and ntag == 0
        assert hits == [(k, i, single[0][1][b]) for i, b in enumerate(mine) for k in range(KT + 1)]
        with _Buffers(nat.gpu) as buf:                                                           # 17 * 65 hits > cap = rows: both wrappers call twice
            assert nat.scan_keys_device([D["a"]] * (KT + 1), 65, buf.up(_bytes_array(files)), buf.up(_bytes_array(seals))) == (status, hits, ntag)
    finally:
        assert tl.bppp_test_rp_set_flat_chunk(nat.h, 0) == 0


# ----------------------------------------------------------------------------- 5. every argument error; rows == 0
@pytest.mark.parametrize("name", NAMES)
def test_scan_keys_argument_errors(gpu, oracle_lib, handles, name):
    D, nat = _data(oracle_lib, name), handles(name)
    keys, single, KT = _expect(oracle_lib, handles, name)
    lib, vp = nat.gpu.lib, lambda x: C.c_void_p(x.ctypes.data)
    files, seals = _bytes_array(D["scan_files"][:2]), _bytes_array(D["scan_seals"][:2])
    status, hk, hr = np.zeros(2, dtype=np.uint32), np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
    nhits, ntag = C.c_size_t(7), C.c_uint64(7)
    good = capi.scalars_to_array(keys[:4])
    call = lambda fn, nk, sec, rows, f, s, cap, k, r, nh: fn(nat.h, nk, sec, rows, f, s, vp(status), cap, k, r, None, None, None, nh, C.byref(ntag))
    for fn in (lib.bppp_rp_scan_keys, lib.bppp_rp_scan_keys_device):
        for bad in (0, N, 2**256 - 1):
            for at in (0, 3):
                sec = capi.scalars_to_array([bad if k == at else keys[k] for k in range(4)])
                for rows in (0, 2):
                    assert call(fn, 4, vp(sec), rows, vp(files), vp(seals), 8, vp(hk), vp(hr), C.byref(nhits)) == ERR_ARG, (bad, at, rows)
                    assert _last_error(nat).startswith("rp_scan_keys: key %d: " % at), _last_error(nat)
            both = capi.scalars_to_array([keys[0], bad, keys[2], bad])                           # the lowest index is named
            assert call(fn, 4, vp(both), 2, vp(files), vp(seals), 8, vp(hk), vp(hr), C.byref(nhits)) == ERR_ARG
            assert _last_error(nat).startswith("rp_scan_keys: key 1: ")
        assert call(fn, 0, vp(good), 2, vp(files), vp(seals), 8, vp(hk), vp(hr), C.byref(nhits)) == ERR_ARG            # no key
        assert call(fn, 2**20 + 1, vp(good), 2, vp(files), vp(seals), 8, vp(hk), vp(hr), C.byref(nhits)) == ERR_ARG    # more than BPPP_RP_SCAN_MAX_KEYS
        assert call(fn, 4, None, 2, vp(files), vp(seals), 8, vp(hk), vp(hr), C.byref(nhits)) == ERR_ARG
        assert call(fn, 4, vp(good), 2, None, vp(seals), 8, vp(hk), vp(hr), C.byref(nhits)) == ERR_ARG
        assert call(fn, 4, vp(good), 2, vp(files), None, 8, vp(hk), vp(hr), C.byref(nhits)) == ERR_ARG
        assert call(fn, 4, vp(good), 2, vp(files), vp(seals), 8, None, vp(hr), C.byref(nhits)) == ERR_ARG
        assert call(fn, 4, vp(good), 2, vp(files), vp(seals), 8, vp(hk), None, C.byref(nhits)) == ERR_ARG
        assert call(fn, 4, vp(good), 2, vp(files), vp(seals), 8, vp(hk), vp(hr), None) == ERR_ARG                      # nhits is required
        assert call(fn, 4, vp(good), 2**31, vp(files), vp(seals), 8, vp(hk), vp(hr), C.byref(nhits)) == ERR_ARG
        # rows == 0: the secrets are judged, nothing else is looked at
        hk[:] = 0xA5; hr[:] = 0xA5
        assert call(fn, 4, vp(good), 0, None, None, 8, vp(hk), vp(hr), C.byref(nhits)) == 0 and nhits.value == 0 and ntag.value == 0
        assert not hk.any() and not hr.any()
    with pytest.raises(capi.BpppError, match="rp_scan_keys: key 1: "):
        nat.scan_keys([keys[0], 0], D["scan_files"][:2], D["scan_seals"][:2])
    _check(_raw(nat, D, keys[:4], 2, 8, device=True), _want(single, 4, 2), 8, D["nr"])           # and after all that the handle still answers
