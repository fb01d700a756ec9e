"""bppp_rp_seal*, bppp_rp_scan*: outputs sealed to a view key, and the scan that finds them again with their openings.

The reference side is rangeproof.seal_host / scan_host over the oracle backend (hashlib and Python integers; never the library under test).  One
data set of 257 rows per setup (rec_test: typed, bin_test: binary, 3 ranges each) is computed once and shared; the smaller row counts are its
prefixes.  Row b is of kind b % 8: owned; sealed to another key; owned; a hint with a bad sign byte; a hint whose x has no point; a flipped memo
bit; two commitments swapped; a commitment whose x has no point — and row 9 is a genuine tag collision, a row sealed to the other key whose view
tag matches under ours, found by a seeded search over r (about 256 tries expected; the fixture fails beyond 4096)."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import capi, encoding
from bulletproofspp_amd import rangeproof as RP
from rp_backends import OracleBackend
from test_gpu_commit_open import _case, _native, _no_point_x, _set_x

pytestmark = pytest.mark.gpu

N = O.N
ERR_ARG = -1
ROWS = 257
COUNTS = (1, 2, 63, 64, 65, 257)
NAMES = ["rec_test", "bin_test"]
FOREIGN, OWNED, BAD_HINT, TAG_ONLY = RP.SCAN_FOREIGN, RP.SCAN_OWNED, RP.SCAN_BAD_HINT, RP.SCAN_TAG_ONLY
COLLISION_ROW = 9
_DATA = {}


def _commit_file(ec, st, outputs, blinds):
    g, H0, B = RP._excess_bases(st)
    return [ec.inner_product([(v % N, g), (bl, B)] + ([(ty % N, H0)] if H0 is not None and ty % N else [])) for (v, ty), bl in zip(outputs, blinds)]


def _data(oracle_lib, name):
    if name in _DATA:
        return _DATA[name]
    ec, be = oracle_lib, OracleBackend(oracle_lib)
    st, inputs = _case(oracle_lib, name)[:2]
    g, H0, B = RP._excess_bases(st)
    typed, nr = H0 is not None, len(st.rds)
    rng = random.Random("seal scan " + name)
    a, other = rng.randrange(1, N), rng.randrange(1, N)
    A, A2 = ec.mul(a, B), ec.mul(other, B)
    keys = [RP.excess_key33(A), RP.excess_key33(A2)]
    # the collision: r with the same view tag under both keys
    tries, r_hit = 0, None
    while r_hit is None:
        tries += 1
        assert tries <= 4096, "no tag collision in 4096 tries"
        r = rng.randrange(1, N)
        r33 = RP.excess_key33(ec.mul(r, B))
        if RP.seal_view_tag(b"", RP.seal_shared(b"", ec.mul(r, A), r33)) == RP.seal_view_tag(b"", RP.seal_shared(b"", ec.mul(r, A2), r33)):
            r_hit = r
    no_x = _no_point_x(ec)
    view_keys, eph, outputs, seals, blinds, files = [], [], [], [], [], []
    for b in range(ROWS):
        kind = b % 8
        src = inputs[b % len(inputs)]
        outs = [(t[0], t[1] if typed else 0) for t in src]
        to_other = kind == 1 or b == COLLISION_ROW
        r = r_hit if b == COLLISION_ROW else rng.randrange(1, N)
        status, seal, bl = RP.seal_host(be, st, keys[1] if to_other else keys[0], r, outs)
        assert status == RP.SEAL_OK
        view_keys.append(keys[1] if to_other else keys[0]); eph.append(r); outputs.append(outs); seals.append(seal); blinds.append(bl)
        files.append(encoding.encode_commitments(_commit_file(ec, st, outs, bl)))
    # the rows the scanner sees: the sealed rows, damaged by kind
    scan_seals, scan_files = list(seals), list(files)
    for b in range(ROWS):
        kind = b % 8
        if b == COLLISION_ROW:
            continue
        if kind == 3:
            scan_seals[b] = seals[b][:32] + b"\x02" + seals[b][33:]
        elif kind == 4:
            scan_seals[b] = encoding.put_field(no_x) + seals[b][32:]
        elif kind == 5:
            s = bytearray(seals[b]); s[34 + 64 * (b % nr) + (b % 64)] ^= 1 << (b % 8); scan_seals[b] = bytes(s)
        elif kind == 6:
            pts = _commit_file(ec, st, outputs[b], blinds[b])
            scan_files[b] = encoding.encode_commitments([pts[1], pts[0]] + pts[2:])
        elif kind == 7:
            scan_files[b] = _set_x(files[b], nr, b % nr, no_x)
    want = [RP.scan_host(be, st, a, f, s) for f, s in zip(scan_files, scan_seals)]
    by_kind = {0: OWNED, 2: OWNED, 3: BAD_HINT, 4: BAD_HINT, 5: TAG_ONLY, 6: TAG_ONLY, 7: TAG_ONLY}
    for b, (verdict, opening) in enumerate(want):
        if b == COLLISION_ROW:
            assert verdict == TAG_ONLY
        elif b % 8 == 1:
            assert verdict in (FOREIGN, TAG_ONLY)
        else:
            assert verdict == by_kind[b % 8], b
        assert opening == ([(v % N, ty, bl) for (v, ty), bl in zip(outputs[b], blinds[b])] if verdict == OWNED else [(0, 0, 0)] * nr)
    _DATA[name] = dict(st=st, a=a, other=other, view_keys=view_keys, eph=eph, outputs=outputs, seals=seals, blinds=blinds, files=files, scan_seals=scan_seals,
                       scan_files=scan_files, want=want, nr=nr, typed=typed, tries=tries)
    return _DATA[name]


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


class _Buffers:
    """device buffers of one call, freed together; outputs are pre-filled with 0xA5"""

    def __init__(self, g):
        self.g, self.ptrs = g, []

    def up(self, arr):
        p = self.g.to_device(np.ascontiguousarray(arr))
        self.ptrs.append(p)
        return p

    def out(self, nbytes):
        return self.up(np.full(max(nbytes, 8), 0xA5, dtype=np.uint8))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.g.free(p)


def _bytes_array(rows):
    return np.frombuffer(b"".join(rows), dtype=np.uint8)


# ----------------------------------------------------------------------------- 1. seals and blindings, byte for byte; host = device
@pytest.mark.parametrize("name", NAMES)
def test_seal_equals_host(gpu, oracle_lib, handles, name):
    D, nat = _data(oracle_lib, name), handles(name)
    nr, sb, g = D["nr"], RP.SEAL_BYTES(D["nr"]), nat.gpu
    for rows in COUNTS:
        seals, blinds, status = nat.seal(D["view_keys"][:rows], D["eph"][:rows], D["outputs"][:rows], want_status=True)
        assert status == [0] * rows and seals == D["seals"][:rows] and blinds == D["blinds"][:rows], rows
        with _Buffers(g) as buf:
            amt = capi.scalars_to_array([v % 2**256 for row in D["outputs"][:rows] for v, _ in row])
            typ = capi.scalars_to_array([t for row in D["outputs"][:rows] for _, t in row])
            d_seals, d_blinds = buf.out(rows * sb), buf.out(rows * nr * 32)
            st = nat.seal_device(rows, buf.up(_bytes_array(D["view_keys"][:rows])), buf.up(capi.scalars_to_array(D["eph"][:rows])), buf.up(amt),
                                 buf.up(typ) if D["typed"] else 0, d_seals, d_blinds, want_status=True)
            assert list(st) == [0] * rows
            raw = g.download(d_seals, (rows * sb,), np.uint8).tobytes()
            assert [raw[b * sb:(b + 1) * sb] for b in range(rows)] == seals, rows
            assert capi.array_to_scalars(g.download(d_blinds, (rows * nr, 4), np.uint64)) == [x for row in blinds for x in row], rows


# ----------------------------------------------------------------------------- 2. the scan against scan_host; host = device; passes; poison
@pytest.mark.parametrize("name", NAMES)
def test_scan_equals_host(gpu, oracle_lib, handles, name):
    D, nat = _data(oracle_lib, name), handles(name)
    nr, sb, cb, g, tl = D["nr"], RP.SEAL_BYTES(D["nr"]), nat.shape["coms_bytes"], nat.gpu, capi.load_test_library()
    assert D["tries"] <= 4096 and D["want"][COLLISION_ROW][0] == TAG_ONLY
    try:
        for rows in COUNTS:
            want = D["want"][:rows]
            want_status, want_open = [v for v, _ in want], [o for _, o in want]
            poisoned = C.c_uint64(0)
            assert tl.bppp_test_rp_poison(nat.h, 0xEE, C.byref(poisoned)) == 0
            status, openings, nowned = nat.scan(D["a"], D["scan_files"][:rows], D["scan_seals"][:rows])
            assert status == want_status and openings == want_open and nowned == want_status.count(OWNED), rows
            # a flat chunk that forces at least three passes (whole rows a pass), over poisoned workspace
            if rows >= 3:
                assert tl.bppp_test_rp_set_flat_chunk(nat.h, nr * max(1, rows // 4)) == 0
                assert tl.bppp_test_rp_poison(nat.h, 0x5C, C.byref(poisoned)) == 0 and poisoned.value > 0
            with _Buffers(g) as buf:
                outs = [buf.out(rows * nr * 32) for _ in range(3)]
                st, n_own = nat.scan_device(D["a"], rows, buf.up(_bytes_array(D["scan_files"][:rows])), buf.up(_bytes_array(D["scan_seals"][:rows])), *outs)
                assert list(st) == want_status and n_own == nowned, rows
                v, t, bl = (capi.array_to_scalars(g.download(o, (rows * nr, 4), np.uint64)) for o in outs)
                assert [[(v[b * nr + i], t[b * nr + i], bl[b * nr + i]) for i in range(nr)] for b in range(rows)] == want_open, rows
                # no output array at all: the verdicts alone
                st2, _ = nat.scan_device(D["a"], rows, buf.ptrs[3], buf.ptrs[4])
                assert list(st2) == want_status
            assert tl.bppp_test_rp_set_flat_chunk(nat.h, 0) == 0
        # under the other secret the two kinds swap: its rows are owned, ours are foreign (or, one in 256, tag only)
        status, _, _ = nat.scan(D["other"], D["scan_files"][:16], D["scan_seals"][:16])
        assert status[1] == OWNED and status[COLLISION_ROW] == OWNED and status[0] in (FOREIGN, TAG_ONLY) and status[3] == BAD_HINT
    finally:
        assert tl.bppp_test_rp_set_flat_chunk(nat.h, 0) == 0


# ----------------------------------------------------------------------------- 3. every refusal of a seal, with and without a status array
@pytest.mark.parametrize("name", NAMES)
def test_seal_refusals(gpu, oracle_lib, handles, name):
    D, nat, be = _data(oracle_lib, name), handles(name), OracleBackend(oracle_lib)
    nr, sb, st = D["nr"], RP.SEAL_BYTES(D["nr"]), D["st"]
    keys, eph, outs = list(D["view_keys"][:8]), list(D["eph"][:8]), [list(r) for r in D["outputs"][:8]]
    keys[1] = keys[1][:32] + b"\x02"                                        # a sign byte above 1
    keys[2] = encoding.put_field(_no_point_x(oracle_lib)) + b"\x00"         # an x without a point
    eph[3] = N                                                               # r = n
    eph[4] = 0                                                               # r = 0
    keys[5], eph[5] = keys[1], 0                                             # the key is judged first
    if D["typed"]:
        outs[6][1] = (outs[6][1][0], N)                                      # a type = n
        eph[7], outs[7][0] = 0, (outs[7][0][0], N + 1)                       # not canonical before zero
    want = [RP.seal_host(be, st, k, r, o) for k, r, o in zip(keys, eph, outs)]
    codes = [0, RP.EXCESS_BAD_KEY, RP.EXCESS_BAD_KEY, RP.SEAL_NOT_CANONICAL, RP.SEAL_ZERO, RP.EXCESS_BAD_KEY] + ([RP.SEAL_NOT_CANONICAL] * 2 if D["typed"] else [0, 0])
    assert [w[0] for w in want] == codes
    seals, blinds, status = nat.seal(keys, eph, outs, want_status=True)
    assert status == codes and seals == [w[1] for w in want] and blinds == [w[2] for w in want]
    assert all(seals[b] == bytes(sb) and blinds[b] == [0] * nr for b in range(8) if codes[b])
    with pytest.raises(capi.BpppError, match="rp_seal: row 1: "):
        nat.seal(keys, eph, outs)
    # the host variant still writes the complete output next to that error
    amt = capi.scalars_to_array([v % 2**256 for row in outs for v, _ in row])
    typ = capi.scalars_to_array([t for row in outs for _, t in row])
    kb, e = _bytes_array(keys), capi.scalars_to_array(eph)
    out_s, out_b = np.full(8 * sb, 0xA5, dtype=np.uint8), np.full((8 * nr, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    vp = lambda x: C.c_void_p(x.ctypes.data)
    lib = nat.gpu.lib
    assert lib.bppp_rp_seal(nat.h, 8, vp(kb), vp(e), vp(amt), vp(typ), vp(out_s), vp(out_b), None) == ERR_ARG
    assert out_s.tobytes() == b"".join(seals) and capi.array_to_scalars(out_b) == [x for row in blinds for x in row]
    # argument errors
    for args in ((None, vp(e), vp(amt), vp(typ), vp(out_s), vp(out_b)), (vp(kb), None, vp(amt), vp(typ), vp(out_s), vp(out_b)), (vp(kb), vp(e), None, vp(typ), vp(out_s), vp(out_b)),
                 (vp(kb), vp(e), vp(amt), vp(typ), None, vp(out_b)), (vp(kb), vp(e), vp(amt), vp(typ), vp(out_s), None)):
        assert lib.bppp_rp_seal(nat.h, 8, *args, None) == ERR_ARG
        assert lib.bppp_rp_seal_device(nat.h, 8, *args, None) == ERR_ARG
    if D["typed"]:
        assert lib.bppp_rp_seal(nat.h, 8, vp(kb), vp(e), vp(amt), None, vp(out_s), vp(out_b), None) == ERR_ARG        # types: NULL only on a binary handle ...
    else:
        good = nat.seal(D["view_keys"][:2], D["eph"][:2], D["outputs"][:2])
        a2 = capi.scalars_to_array([v % 2**256 for row in D["outputs"][:2] for v, _ in row])
        assert lib.bppp_rp_seal(nat.h, 2, vp(_bytes_array(D["view_keys"][:2])), vp(capi.scalars_to_array(D["eph"][:2])), vp(a2), None, vp(out_s), vp(out_b), None) == 0
        assert out_s.tobytes()[:2 * sb] == b"".join(good[0])                                                         # ... where it is allowed
    assert lib.bppp_rp_seal(nat.h, 0, None, None, None, None, None, None, None) == 0
    assert lib.bppp_rp_seal(nat.h, 2**31, vp(kb), vp(e), vp(amt), vp(typ), vp(out_s), vp(out_b), None) == ERR_ARG


# ----------------------------------------------------------------------------- 4. every argument error of a scan
@pytest.mark.parametrize("name", NAMES)
def test_scan_argument_errors(gpu, oracle_lib, handles, name):
    D, nat = _data(oracle_lib, name), handles(name)
    lib, vp = nat.gpu.lib, lambda x: C.c_void_p(x.ctypes.data)
    files, seals = _bytes_array(D["scan_files"][:2]), _bytes_array(D["scan_seals"][:2])
    status, nown = np.zeros(2, dtype=np.uint32), C.c_size_t(7)
    a = capi.int_to_limbs(D["a"])
    for bad in (0, N, N + 5, 2**256 - 1):
        for rows in (0, 2):
            assert lib.bppp_rp_scan(nat.h, vp(capi.int_to_limbs(bad)), rows, vp(files), vp(seals), vp(status), None, None, None, C.byref(nown)) == ERR_ARG, (bad, rows)
        with pytest.raises(capi.BpppError, match="view secret"):
            nat.scan(bad, D["scan_files"][:2], D["scan_seals"][:2])
    assert lib.bppp_rp_scan(nat.h, None, 2, vp(files), vp(seals), vp(status), None, None, None, None) == ERR_ARG
    assert lib.bppp_rp_scan(nat.h, vp(a), 2, None, vp(seals), vp(status), None, None, None, None) == ERR_ARG
    assert lib.bppp_rp_scan(nat.h, vp(a), 2, vp(files), None, vp(status), None, None, None, None) == ERR_ARG
    assert lib.bppp_rp_scan(nat.h, vp(a), 2, vp(files), vp(seals), None, None, None, None, None) == ERR_ARG
    assert lib.bppp_rp_scan_device(nat.h, vp(a), 2, None, None, vp(status), None, None, None, None) == ERR_ARG
    assert lib.bppp_rp_scan(nat.h, vp(a), 2**31, vp(files), vp(seals), vp(status), None, None, None, None) == ERR_ARG
    assert lib.bppp_rp_scan(nat.h, vp(a), 0, None, None, None, None, None, None, C.byref(nown)) == 0 and nown.value == 0
    assert lib.bppp_rp_scan(nat.h, vp(a), 2, vp(files), vp(seals), vp(status), None, None, None, None) == 0 and list(status) == [OWNED, D["want"][1][0]]


# ----------------------------------------------------------------------------- 5. the prover takes the sealed blindings as they are
@pytest.mark.parametrize("name", NAMES)
def test_prove_with_sealed_blindings(gpu, oracle_lib, handles, name):
    D, nat = _data(oracle_lib, name), handles(name)
    inputs = _case(oracle_lib, name)[1]
    B = 4
    rows = [[(t[0], t[1], bl) if D["typed"] else (t[0], bl) for t, bl in zip(inputs[b], D["blinds"][b])] for b in range(B)]
    proved = nat.prove_batch(rows, [b"sealed blinds %03d" % b for b in range(B)])
    coms = [c for c, _ in proved]
    assert coms == D["files"][:B]
    assert nat.verify_batch(coms, [p for _, p in proved], hashlib.sha256(b"seal scan verify").digest())
    status, openings, nowned = nat.scan(D["a"], coms, D["seals"][:B])
    want = [OWNED if b % 8 != 1 else D["want"][b][0] for b in range(B)]
    assert status == want and nowned == want.count(OWNED)
    for b in range(B):
        if want[b] == OWNED:
            assert openings[b] == [(v % N, ty, bl) for (v, ty), bl in zip(D["outputs"][b], D["blinds"][b])]
