"""The passes of the balance calls that the tally's chunk does not plan: bppp_rp_commit_batch, bppp_rp_open_each, bppp_rp_open_batch,
bppp_rp_excess_sign, bppp_rp_excess_keys, bppp_rp_excess_verify_keys_each, bppp_rp_excess_verify_keys_batch.  Each takes one pass over its workspace
for up to 2^22 (the key calls 2^20) items, so no other test comes back for a second; bppp_test_rp_set_flat_chunk lowers that.

Every case runs 7 items once at the default and once with passes of 3, 3 and 1, and wants every output byte for byte the same: files, signatures, keys,
statuses, accept, excess points, and the combined point (the weights depend on index_offset + position only, so the passes' points add up to the one-pass
point).  The item at position 4, in the second pass, is bad, so an offset that is wrong from the second pass on shows in the statuses and the batches
fall through to their exact pass.  Whether the default-chunk results are right is the business of test_gpu_commit_open, test_gpu_excess and
test_gpu_excess_keys, whose fixtures these are."""
import hashlib

import pytest

import pyoracle as O
from bulletproofspp_amd import capi
from test_gpu_commit_open import _case, handles  # noqa: F401  (handles: the module's fixture, one native handle per setup)

pytestmark = pytest.mark.gpu

N = O.N
SEED = hashlib.sha256(b"flat chunk seed").digest()
AUX = hashlib.sha256(b"flat chunk aux").digest()
NAMES = ["32bit", "bin_test"]                # typed and binary at the fewest ranges the shared fixtures have (1 and 3)
ITEMS, PASS, BAD = 7, 3, 4
OK, MISMATCH, NOT_CANONICAL = 0, 1, 3


def _twice(nat, chunk, call):
    """call () at the default chunk, then with `chunk` items a pass; the hook is restored whatever happens"""
    tl = capi.load_test_library()
    want = call()
    try:
        assert tl.bppp_test_rp_set_flat_chunk(nat.h, chunk) == 0
        got = call()
    finally:
        assert tl.bppp_test_rp_set_flat_chunk(nat.h, 0) == 0
    return want, got


def _rows(oracle_lib, name):
    """7 valid rows and their files; commit / open take max (1, chunk / nranges) rows a pass"""
    st, inputs, _, _, files = _case(oracle_lib, name)
    return [list(r) for r in inputs[:ITEMS]], list(files[:ITEMS]), PASS * len(st.rds)


def _bad_blinding(rows):
    rows[BAD][-1] = rows[BAD][-1][:-1] + (N,)             # typed (v, ty, bl), binary (v, bl): the blinding is last
    return rows


def _blinds():
    es = [int.from_bytes(hashlib.sha256(b"flat chunk e %d" % t).digest(), "big") % (N - 1) + 1 for t in range(ITEMS)]
    return es, [hashlib.sha256(b"flat chunk msg %d" % t).digest() for t in range(ITEMS)]


def _signed(nat):
    """7 keys, messages and signatures (made at the default chunk), the signature at BAD with the last byte of s flipped"""
    es, msgs = _blinds()
    sigs, keys = nat.excess_sign(es, msgs, AUX), nat.excess_keys(es)
    sigs[BAD] = sigs[BAD][:-1] + bytes([sigs[BAD][-1] ^ 1])
    return keys, msgs, sigs


def _one_bad(code):
    return [code if t == BAD else OK for t in range(ITEMS)]


@pytest.mark.parametrize("name", NAMES)
def test_commit(gpu, oracle_lib, handles, name):
    nat = handles(name)
    rows, files, chunk = _rows(oracle_lib, name)
    want, got = _twice(nat, chunk, lambda: nat.commit_batch(_bad_blinding(rows), want_status=True))
    assert got == want
    assert [f for t, f in enumerate(want[0]) if t != BAD] == [f for t, f in enumerate(files) if t != BAD] and want[0][BAD] is None
    assert [s != 0 for s in want[1]] == [t == BAD for t in range(ITEMS)]


@pytest.mark.parametrize("name", NAMES)
def test_open_each(gpu, oracle_lib, handles, name):
    nat = handles(name)
    rows, files, chunk = _rows(oracle_lib, name)
    nr = len(rows[0])
    rows[BAD][nr - 1] = (rows[BAD][nr - 1][0] + 1,) + rows[BAD][nr - 1][1:]               # a wrong amount
    want, got = _twice(nat, chunk, lambda: nat.open_each(files, rows))
    assert got == want == [[MISMATCH if (b, i) == (BAD, nr - 1) else OK for i in range(nr)] for b in range(ITEMS)]


@pytest.mark.parametrize("name", NAMES)
def test_open_batch(gpu, oracle_lib, handles, name):
    nat = handles(name)
    rows, files, chunk = _rows(oracle_lib, name)
    nr = len(rows[0])
    good = _twice(nat, chunk, lambda: nat.open_batch(files, rows, SEED, want_status=True, want_point=True))
    assert good[1] == good[0] == (True, [[OK] * nr] * ITEMS, None)
    rows[BAD][0] = (rows[BAD][0][0] + 1,) + rows[BAD][0][1:]
    want, got = _twice(nat, chunk, lambda: nat.open_batch(files, rows, SEED, want_status=True, want_point=True))
    assert got == want
    assert want[0] is False and want[2] is not None and want[1] == [[MISMATCH if (b, i) == (BAD, 0) else OK for i in range(nr)] for b in range(ITEMS)]


@pytest.mark.parametrize("name", NAMES)
def test_sign(gpu, oracle_lib, handles, name):
    nat = handles(name)
    es, msgs = _blinds()
    good = _twice(nat, PASS, lambda: nat.excess_sign(es, msgs, AUX, want_status=True, want_points=True))
    assert good[1] == good[0] and good[0][1] == [OK] * ITEMS and None not in good[0][2] and len(set(good[0][0])) == ITEMS
    es[BAD] = N
    want, got = _twice(nat, PASS, lambda: nat.excess_sign(es, msgs, AUX, want_status=True, want_points=True))
    assert got == want
    assert want[1] == _one_bad(capi.RP_EXCESS_NOT_CANONICAL) and want[0][BAD] == bytes(65) and want[2][BAD] is None
    assert [want[k][t] for k in (0, 2) for t in range(ITEMS) if t != BAD] == [good[0][k][t] for k in (0, 2) for t in range(ITEMS) if t != BAD]


@pytest.mark.parametrize("name", NAMES)
def test_keys(gpu, oracle_lib, handles, name):
    nat = handles(name)
    es, _ = _blinds()
    es[BAD] = N
    want, got = _twice(nat, 4 * PASS, lambda: nat.excess_keys(es, want_status=True))     # a quarter of the chunk is a pass of keys
    assert got == want
    assert want[1] == _one_bad(capi.RP_EXCESS_NOT_CANONICAL) and want[0][BAD] == bytes(33) and len(set(want[0])) == ITEMS


@pytest.mark.parametrize("name", NAMES)
def test_verify_keys_each(gpu, oracle_lib, handles, name):
    nat = handles(name)
    keys, msgs, sigs = _signed(nat)
    want, got = _twice(nat, 4 * PASS, lambda: nat.excess_verify_keys_each(keys, msgs, sigs))
    assert got == want == _one_bad(MISMATCH)


@pytest.mark.parametrize("name", NAMES)
def test_verify_keys_batch(gpu, oracle_lib, handles, name):
    nat = handles(name)
    keys, msgs, sigs = _signed(nat)
    want, got = _twice(nat, 4 * PASS, lambda: nat.excess_verify_keys_batch(keys, msgs, sigs, SEED, want_status=True, want_point=True))
    assert got == want
    assert want[0] is False and want[1] == _one_bad(MISMATCH) and want[2] is not None


@pytest.mark.parametrize("name", NAMES)
def test_a_refusal_without_a_status_array_names_its_position(gpu, oracle_lib, handles, name):
    """the first refusal is the call's error: position 4 of the job, not 1 of the second pass"""
    nat = handles(name)
    rows, _, chunk = _rows(oracle_lib, name)
    es, msgs = _blinds()
    es[BAD] = N
    calls = [(chunk, lambda: nat.commit_batch(_bad_blinding(rows)), r"rp_commit_batch: proof 4: "),
             (PASS, lambda: nat.excess_sign(es, msgs, AUX), r"rp_excess_sign: sum 4: .*not canonical"),
             (4 * PASS, lambda: nat.excess_keys(es), r"rp_excess_keys: sum 4: .*not canonical")]
    tl = capi.load_test_library()
    for items, call, text in calls:
        try:
            assert tl.bppp_test_rp_set_flat_chunk(nat.h, items) == 0
            with pytest.raises(capi.BpppError, match=text):
                call()
        finally:
            assert tl.bppp_test_rp_set_flat_chunk(nat.h, 0) == 0
