"""bppp_rp_verify_block*: the range proofs of a block's new outputs, its kernel signatures against their stated keys and its sums after cut-through
in one call and ONE MSM.

The reference side is the three existing calls under rangeproof.block_seeds(seed) — bppp_rp_verify_bound for V, bppp_rp_excess_verify_keys_batch for K,
bppp_rp_excess_sums_batch for S — their points added by the CPU oracle's group law (pyoracle), and, for the statuses of a rejected block, verify_each,
excess_verify_keys_each and excess_sums_each over the same inputs.  One block per setup is built once and shared: 9 pool rows with the first 5 proven,
3 sums of (entries, keys) = (4, 1), (3, 2), (2, 0), 3 keys.  Every job is a handful of proofs."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import array_to_point, load_test_library
import test_gpu_prove_device as PD
from test_gpu_commit_open import _no_point_x, _set_x
from test_gpu_excess_keys import _s_of, _with_s

pytestmark = pytest.mark.gpu

N = O.N
TAG = b"block test"
SEED = hashlib.sha256(b"block seed").digest()
SEED2 = hashlib.sha256(b"another block seed").digest()
AUX = hashlib.sha256(b"block aux").digest()
NAMES = ["32bit", "rec_test", "bin_test"]            # inner-product flavour; typed, norm-linear; binary
ROWS, NPROOFS = 9, 5
SHAPES = [(4, 1), (3, 2), (2, 0)]
VALID, INVALID, PROOF_MALFORMED = 0, 1, 2
OK, MISMATCH, MALFORMED, NOT_CANONICAL, BAD_R, NO_KEY, BAD_KEY = 0, 1, 2, 3, 4, 5, 6
ERR_ARG = -1
_BLOCKS, _XS = {}, {}


class Block:
    """the arguments of one verify_block call; copy() for a mutation"""
    FIELDS = ("coms", "proofs", "ss", "en", "claims", "ks", "keys", "msgs", "sigs", "bindings")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw[f])

    def copy(self):
        return Block(**{f: list(getattr(self, f)) if getattr(self, f) is not None else None for f in self.FIELDS})

    def args(self):
        return (self.coms, self.proofs, self.ss, self.en, self.claims, self.ks, self.keys, self.msgs, self.sigs)


@pytest.fixture(scope="module")
def handles(gpu):
    made = {}

    def get(name, tag=TAG):
        if (name, tag) not in made:
            st = PD._setup(gpu, name)
            nat = (BRP.NativeBinaryRangeProofs if isinstance(st, BRP.SetupBRP) else RP.NativeRangeProofs)(gpu, st, oracle_tag=tag)
            nat.set_option("comb_min", 1)
            nat.set_option("comb_bits", PD.BITS)
            made[(name, tag)] = nat
        return made[(name, tag)]
    yield get
    for nat in made.values():
        nat.close()


def _block(handles, name, bound=True):
    """the valid block of a setup (computed once): B spent inside it is not modelled here — the sums are random signed selections whose claims and
    keys are made to balance"""
    key = (name, bound)
    if key in _BLOCKS:
        return _BLOCKS[key]
    nat = handles(name)
    st, binary = nat.st, name == "bin_test"
    nr = len(st.rds)
    inputs = PD._inputs(name, st, ROWS, 17)
    bindings = [hashlib.sha256(b"block binding %d" % b).digest() for b in range(NPROOFS)] if bound else None
    files = nat.prove_batch(inputs, PD._prefixes(ROWS, b"block " + name.encode()), bindings=(bindings + [bytes(32)] * (ROWS - NPROOFS)) if bound else None)
    coms, proofs = [c for c, _ in files], [p for _, p in files][:NPROOFS]
    flat = [((r[0], 0, r[1]) if binary else tuple(r)) for row in inputs for r in row]       # (amount, type, blinding) of flat index row * nranges + i
    rng = random.Random("block " + name)
    total = ROWS * nr
    # every sum touches a proven row and an unproven one
    ss, en, ks, xs, claims = [0], [], [0], [], []
    for t, (ne, nk) in enumerate(SHAPES):
        picks = [(rng.randrange(NPROOFS * nr), False), (NPROOFS * nr + rng.randrange(total - NPROOFS * nr), True)] + [(rng.randrange(total), rng.random() < 0.5) for _ in range(ne - 2)]
        en += [RP.tally_entry(j, sub) for j, sub in picks]
        ss.append(len(en))
        a, ty, e = RP.tally_claims_host(flat, [0, ne], [RP.tally_entry(j, sub) for j, sub in picks])[0]
        mine = [rng.randrange(1, N) for _ in range(nk)]
        off = (e - sum(mine)) % N
        xs += mine
        ks.append(len(xs))
        claims.append((a, off) if binary else (a, ty, off))
    msgs = [hashlib.sha256(b"block msg %d" % k).digest() for k in range(len(xs))]
    blk = Block(coms=coms, proofs=proofs, ss=ss, en=en, claims=claims, ks=ks, keys=nat.excess_keys(xs), msgs=msgs, sigs=nat.excess_sign(xs, msgs, AUX), bindings=bindings)
    _BLOCKS[key], _XS[name] = blk, xs
    return blk


def _parts(nat, gpu, blk, seed):
    """(V, K, S) of the three existing calls under block_seeds(seed), as points"""
    s0, s1, s2 = RP.block_seeds(seed)
    n = len(blk.proofs)
    V = None
    if n:
        cb, pb = (np.frombuffer(b"".join(x), dtype=np.uint8) for x in (blk.coms[:n], blk.proofs))
        bd = np.frombuffer(b"".join(blk.bindings), dtype=np.uint8) if blk.bindings is not None else None
        acc, xy, sd = C.c_int(-1), np.zeros(8, dtype=np.uint64), np.frombuffer(s0, dtype=np.uint8)
        vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        assert gpu.lib.bppp_rp_verify_bound(nat.h, n, vp(cb), vp(pb), None, vp(bd), vp(sd), C.byref(acc), None, None, vp(xy)) == 0
        V = array_to_point(xy)
    K = nat.excess_verify_keys_batch(blk.keys, blk.msgs, blk.sigs, s1, want_point=True)[2] if blk.keys else None
    S = nat.excess_sums_batch(blk.coms, blk.ss, blk.en, blk.claims, blk.ks, blk.keys, s2, want_point=True)[2] if len(blk.ss) > 1 else None
    return V, K, S


def _sum3(ec, pts):
    acc = None
    for p in pts:
        acc = ec.add(acc, p)
    return acc


def _each(nat, blk):
    """the statuses of the three counterparts over the block's inputs"""
    n = len(blk.proofs)
    return (nat.verify_each(blk.coms[:n], blk.proofs, bindings=blk.bindings), nat.excess_verify_keys_each(blk.keys, blk.msgs, blk.sigs),
            nat.excess_sums_each(blk.coms, blk.ss, blk.en, blk.claims, blk.ks, blk.keys))


def _both(nat, blk, seed=SEED, **kw):
    host = nat.verify_block(*blk.args(), bindings=blk.bindings, seed=seed, want_status=True, want_point=True, **kw)
    dev = nat.verify_block_device(*blk.args(), bindings=blk.bindings, seed=seed, want_status=True, want_point=True, **kw)
    assert host == dev
    return host


def _tamper_proof(blk, b):
    p = bytearray(blk.proofs[b])
    p[10] ^= 1                                           # a bit of the first final-witness scalar
    blk.proofs[b] = bytes(p)


def _wrong(handles, name):
    """well-formed but wrong in all three parts: proof 1 tampered in a response scalar, signature 2 with s + 1, the fee of sum 0 off by one"""
    blk = _block(handles, name).copy()
    _tamper_proof(blk, 1)
    blk.sigs[2] = _with_s(blk.sigs[2], (_s_of(blk.sigs[2]) + 1) % N)
    blk.claims[0] = (blk.claims[0][0] + 1,) + tuple(blk.claims[0][1:])
    return blk


def _counts(nat):
    v = [C.c_uint64(0) for _ in range(4)]
    assert load_test_library().bppp_test_rp_last_block_counts(nat.h, *[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


# ----------------------------------------------------------------------------- 1. accept; 4. one MSM, shared lifts
@pytest.mark.parametrize("name", NAMES)
def test_accept_and_counts(gpu, handles, name):
    nat, blk = handles(name), _block(handles, name)
    assert _both(nat, blk) == (True, ([VALID] * NPROOFS, [OK] * 3, [OK] * 3), None)
    assert nat.verify_block(*blk.args(), bindings=blk.bindings) is True                 # a fresh seed
    sh, nr = nat.shape, len(nat.st.rds)
    ninit = (2 if name == "bin_test" else 4) + nr
    terms = 1 + sh["lin_len"] + sh["norm_len"] + NPROOFS * (ninit + 2 * sh["rounds"]) + len(blk.en) + 2 * len(blk.keys)
    assert _counts(nat) == (1, terms, len(blk.keys), ROWS * nr)


# ----------------------------------------------------------------------------- 2. the formula
@pytest.mark.parametrize("name", NAMES)
def test_formula(gpu, oracle_lib, handles, name):
    nat, blk = handles(name), _wrong(handles, name)
    V, K, S = _parts(nat, gpu, blk, SEED)
    assert None not in (V, K, S)
    acc, status, point = _both(nat, blk)
    assert not acc and point == _sum3(oracle_lib, (V, K, S)) and point is not None
    assert status == _each(nat, blk)
    assert status[0][1] == INVALID and status[1][2] == MISMATCH and status[2][0] == MISMATCH
    other = nat.verify_block(*blk.args(), bindings=blk.bindings, seed=SEED2, want_point=True)
    assert other[0] is False and other[2] not in (None, point)
    assert other[2] == _sum3(oracle_lib, _parts(nat, gpu, blk, SEED2))


# ----------------------------------------------------------------------------- 3. each part alone rejects, statuses are the counterparts'
def _proof_x_offset(nat, name):
    sh = nat.shape
    ncoms = (2 if name == "bin_test" else 4) + 2 * sh["rounds"]
    return 32 * (sh["final_norm"] + sh["final_lin"]) + (ncoms + 7) // 8


def _mut_proof(ec, nat, name, blk):
    _tamper_proof(blk, 3)
    return {"proof": {3: INVALID}}


def _mut_swap(ec, nat, name, blk):
    blk.bindings[0], blk.bindings[4] = blk.bindings[4], blk.bindings[0]
    return {"proof": {0: INVALID, 4: INVALID}}


def _mut_proof_x(ec, nat, name, blk):
    o = _proof_x_offset(nat, name)
    blk.proofs[2] = blk.proofs[2][:o] + RP._put(_no_point_x(ec)) + blk.proofs[2][o + 32:]
    return {"proof": {2: PROOF_MALFORMED}}


def _row_of_entry(blk, nr, proven):
    """(sum, row) of the first entry that gathers from a proven (or an unproven) row"""
    for t in range(len(blk.ss) - 1):
        for p in range(blk.ss[t], blk.ss[t + 1]):
            j = blk.en[p] & 0x7FFFFFFF
            if (j // nr < NPROOFS) == proven:
                return t, j // nr, j % nr
    raise AssertionError("the block has such an entry in every sum")


def _sums_that_gather(blk, j):
    return {t: MALFORMED for t in range(len(blk.ss) - 1) if any((e & 0x7FFFFFFF) == j for e in blk.en[blk.ss[t]:blk.ss[t + 1]])}


def _mut_proven_row(ec, nat, name, blk):
    nr = len(nat.st.rds)
    t, row, i = _row_of_entry(blk, nr, True)
    blk.coms[row] = _set_x(blk.coms[row], nr, i, _no_point_x(ec))
    return {"proof": {row: PROOF_MALFORMED}, "sum": _sums_that_gather(blk, row * nr + i)}


def _mut_input_row(ec, nat, name, blk):
    nr = len(nat.st.rds)
    t, row, i = _row_of_entry(blk, nr, False)
    blk.coms[row] = _set_x(blk.coms[row], nr, i, _no_point_x(ec))
    return {"sum": _sums_that_gather(blk, row * nr + i)}


def _mut_s1(ec, nat, name, blk):
    blk.sigs[1] = _with_s(blk.sigs[1], (_s_of(blk.sigs[1]) + 1) % N)
    return {"key": {1: MISMATCH}}


def _mut_sn(ec, nat, name, blk):
    blk.sigs[0] = _with_s(blk.sigs[0], N)
    return {"key": {0: NOT_CANONICAL}}


def _mut_r(ec, nat, name, blk):
    blk.sigs[2] = RP._put(_no_point_x(ec)) + blk.sigs[2][32:]
    return {"key": {2: BAD_R}}


def _mut_key_sign(ec, nat, name, blk):
    blk.keys[1] = blk.keys[1][:32] + b"\x02"
    return {"key": {1: BAD_KEY}, "sum": {1: BAD_KEY}}


def _mut_offset(ec, nat, name, blk):
    blk.claims[2] = tuple(blk.claims[2][:-1]) + (N,)
    return {"sum": {2: NOT_CANONICAL}}


def _mut_fee(ec, nat, name, blk):
    blk.claims[1] = (blk.claims[1][0] + 1,) + tuple(blk.claims[1][1:])
    return {"sum": {1: MISMATCH}}


def _mut_key_moved(ec, nat, name, blk):
    blk.ks[1] = 0                                        # key 0 now belongs to sum 1
    return {"sum": {0: MISMATCH, 1: MISMATCH}}


MUTATIONS = {"proof tampered": _mut_proof, "bindings swapped": _mut_swap, "proof x without a point": _mut_proof_x, "proven row x without a point": _mut_proven_row,
             "input row x without a point": _mut_input_row, "s+1": _mut_s1, "s=n": _mut_sn, "R without a point": _mut_r, "key sign byte 2": _mut_key_sign,
             "offset >= n": _mut_offset, "fee off by one": _mut_fee, "key moved to the other group": _mut_key_moved}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
@pytest.mark.parametrize("name", NAMES)
def test_each_part_alone_rejects(gpu, oracle_lib, handles, name, mutation):
    nat, blk = handles(name), _block(handles, name).copy()
    expect = MUTATIONS[mutation](oracle_lib, nat, name, blk)
    want = ([expect.get("proof", {}).get(b, VALID) for b in range(NPROOFS)], [expect.get("key", {}).get(k, OK) for k in range(3)],
            [expect.get("sum", {}).get(t, OK) for t in range(3)])
    each = _each(nat, blk)
    assert each == want, "the counterparts themselves"
    acc, status, _ = _both(nat, blk)
    assert not acc and status == each
    assert nat.verify_block(*blk.args(), bindings=blk.bindings, seed=SEED) is False     # no status array asked for


def test_culprits_by_one_pass(gpu, handles):
    nat, blk = handles("rec_test"), _wrong(handles, "rec_test")
    want = _both(nat, blk)
    nat.set_option("culprits", 1)
    try:
        assert _both(nat, blk) == want
    finally:
        nat.set_option("culprits", 0)


# ----------------------------------------------------------------------------- 5. shards
def _shard(blk, nr, rows, proofs, sums):
    """the sub-block of pool rows `rows` (a list; its first len(proofs) are the proven ones), and sums [sums[0], sums[1]) with their keys, re-indexed"""
    where = {r: i for i, r in enumerate(rows)}
    t0, t1 = sums
    en = []
    for p in range(blk.ss[t0], blk.ss[t1]):
        j = blk.en[p] & 0x7FFFFFFF
        en.append(RP.tally_entry(where[j // nr] * nr + j % nr, bool(blk.en[p] >> 31)))
    k0, k1 = blk.ks[t0], blk.ks[t1]
    return Block(coms=[blk.coms[r] for r in rows], proofs=[blk.proofs[b] for b in proofs], ss=[s - blk.ss[t0] for s in blk.ss[t0:t1 + 1]], en=en, claims=blk.claims[t0:t1],
                 ks=[k - k0 for k in blk.ks[t0:t1 + 1]], keys=blk.keys[k0:k1], msgs=blk.msgs[k0:k1], sigs=blk.sigs[k0:k1],
                 bindings=[blk.bindings[b] for b in proofs]), k0


@pytest.mark.parametrize("name", NAMES)
def test_shards_add_up(gpu, handles, name):
    """proofs 0, 1 | 2 .. 4, sums 0 | 1, 2 and so keys 0 | 1, 2: both shards carry proofs, keys and sums, and the second shard is wrong in all three
    parts (proof 3, signature 2, the fee of sum 1), so that each of its offsets moves a weight of a term that does not vanish"""
    nat, blk = handles(name), _wrong(handles, name)
    _tamper_proof(blk, 3)
    blk.claims[1] = (blk.claims[1][0] + 1,) + tuple(blk.claims[1][1:])
    nr = len(nat.st.rds)
    whole = _both(nat, blk)[2]
    rest = list(range(NPROOFS, ROWS))
    lo, klo = _shard(blk, nr, [0, 1] + [2, 3, 4] + rest, [0, 1], (0, 1))
    hi, khi = _shard(blk, nr, [2, 3, 4] + [0, 1] + rest, [2, 3, 4], (1, 3))
    assert (klo, khi) == (0, 1) and len(lo.keys) == 1 and len(hi.keys) == 2 and len(lo.ss) == 2 and len(hi.ss) == 3
    p_lo = _both(nat, lo, offsets=(0, klo, 0))[2]
    p_hi = _both(nat, hi, offsets=(2, khi, 1))[2]
    assert None not in (whole, p_lo, p_hi)
    assert gpu.sum_points(capi.points_to_array([p_lo, p_hi])) == whole
    # every offset of the second shard is applied: leaving any one at zero gives another point
    others = [nat.verify_block(*hi.args(), bindings=hi.bindings, seed=SEED, offsets=o, want_point=True)[2] for o in ((0, khi, 1), (2, 0, 1), (2, khi, 0))]
    assert None not in others and len({p_hi, *others}) == 4


# ----------------------------------------------------------------------------- 6. empty parts
@pytest.mark.parametrize("name", NAMES)
def test_empty_parts(gpu, oracle_lib, handles, name):
    nat, blk, ec = handles(name), _wrong(handles, name), oracle_lib
    V, K, S = _parts(nat, gpu, blk, SEED)
    # no proofs: K + S
    b = blk.copy()
    b.proofs, b.bindings = [], None
    acc, status, point = _both(nat, b)
    assert not acc and point == ec.add(K, S) and status[0] == [] and status[1:] == _each(nat, blk)[1:]
    # no keys, key-less sums: V + S'
    b = blk.copy()
    b.keys, b.msgs, b.sigs, b.ks = [], [], [], [0, 0, 0, 0]
    S2 = nat.excess_sums_batch(b.coms, b.ss, b.en, b.claims, b.ks, [], RP.block_seeds(SEED)[2], want_point=True)[2]
    acc, status, point = _both(nat, b)
    assert not acc and point == ec.add(V, S2) and S2 not in (None, S)
    # no sums and no keys: V alone
    b.ss, b.en, b.claims, b.ks = [0], [], [], [0]
    assert _both(nat, b)[2] == V
    # no sums: the keys belong to no sum, V + K
    b = blk.copy()
    b.ss, b.en, b.claims, b.ks = [0], [], [], [0]
    assert _both(nat, b)[2] == ec.add(V, K)
    # all empty: accepted, and nothing else is looked at
    acc = C.c_int(-1)
    xy = np.full(8, 7, dtype=np.uint64)
    empty = capi.RpBlock()
    for fn in (gpu.lib.bppp_rp_verify_block, gpu.lib.bppp_rp_verify_block_device):
        assert fn(nat.h, C.byref(empty), None, C.byref(acc), None, C.c_void_p(xy.ctypes.data)) == 0 and acc.value == 1 and not xy.any()


# ----------------------------------------------------------------------------- 7. errors: no output array is written
def _raw(nat, blk, device, edit=None, bindings=True):
    """a raw call with prefilled outputs -> (rc, error text, outputs untouched)"""
    gpu = nat.gpu
    arrs, n = nat.block_arrays(*blk.args(), blk.bindings if bindings else None)
    c = capi.RpBlock(**n)
    dev = []
    for nm, a in arrs:
        if a is None:
            continue
        if device:
            dev.append(gpu.to_device(a))
            setattr(c, nm, dev[-1])
        else:
            setattr(c, nm, a.ctypes.data)
    if edit:
        edit(c)
    sts = [np.full(8, 77, dtype=np.uint32) for _ in range(3)]
    status = capi.RpBlockStatus(*[a.ctypes.data for a in sts])
    xy, acc, sd = np.full(8, 77, dtype=np.uint64), C.c_int(-5), np.frombuffer(SEED, dtype=np.uint8)
    fn = gpu.lib.bppp_rp_verify_block_device if device else gpu.lib.bppp_rp_verify_block
    rc = fn(nat.h, C.byref(c), C.c_void_p(sd.ctypes.data), C.byref(acc), C.byref(status), C.c_void_p(xy.ctypes.data))
    err = gpu.lib.bppp_last_error(gpu.h).decode()
    for d in dev:
        gpu.free(d)
    return rc, err, all((a == 77).all() for a in sts + [xy]), acc.value


@pytest.mark.parametrize("device", [False, True])
def test_errors(gpu, handles, device):
    nat, good = handles("rec_test"), _block(handles, "rec_test")
    nr = len(nat.st.rds)

    def fails(match, edit=None, blk=good, bindings=True, n=nat):
        rc, err, untouched, acc = _raw(n, blk, device, edit, bindings)
        assert rc == ERR_ARG and match in err and untouched and acc == -5, (rc, err, untouched, acc)

    fails("nproofs", lambda c: setattr(c, "nproofs", ROWS + 1))
    b = good.copy(); b.ss[1] = b.ss[2] + 1
    fails("sum_start[", blk=b)
    b = good.copy(); b.ks[1] = 3; b.ks[2] = 1
    fails("key_start[", blk=b)
    b = good.copy(); b.en[3] = ROWS * nr
    fails("entries[3]", blk=b)
    fails("must be given together", lambda c: setattr(c, "claim_offsets", None))
    fails("null input", lambda c: setattr(c, "sigs", None))
    tl = load_test_library()
    try:
        assert tl.bppp_test_rp_set_tally_chunk(nat.h, len(good.en) + len(good.keys) - 1) == 0
        fails("tally chunk")
        assert "shard it" in _raw(nat, good, device, None)[1]
    finally:
        assert tl.bppp_test_rp_set_tally_chunk(nat.h, 0) == 0
    try:
        assert tl.bppp_test_rp_set_flat_chunk(nat.h, 8) == 0                              # two keys a pass
        fails("flat chunk")
    finally:
        assert tl.bppp_test_rp_set_flat_chunk(nat.h, 0) == 0
    assert _raw(nat, good, device)[::3] == (0, 1)
    before = _counts(nat)
    fails("nproofs", lambda c: setattr(c, "nproofs", ROWS + 1))                            # a refused call leaves the handle's counters as they were
    assert before[0] == 1 and _counts(nat) == before
    # a handle whose tag leaves no room for a binding: refused with bindings, accepted without (over proofs made unbound)
    long_nat = handles("rec_test", b"t" * 40)
    inputs = PD._inputs("rec_test", long_nat.st, ROWS, 17)
    files = long_nat.prove_batch(inputs, PD._prefixes(ROWS, b"block long"))
    b = good.copy()
    b.coms, b.proofs = [c for c, _ in files], [p for _, p in files][:NPROOFS]
    b.sigs = long_nat.excess_sign(_XS["rec_test"], b.msgs, AUX)                          # the challenge hashes the tag; the keys are the same points
    fails("tag too long", blk=b, n=long_nat)
    rc, err, untouched, acc = _raw(long_nat, b, device, bindings=False)
    assert (rc, acc) == (0, 1) and not untouched


# ----------------------------------------------------------------------------- 8. unbound
@pytest.mark.parametrize("name", NAMES)
def test_unbound(gpu, oracle_lib, handles, name):
    nat, blk = handles(name), _block(handles, name, bound=False)
    assert blk.bindings is None
    assert _both(nat, blk) == (True, ([VALID] * NPROOFS, [OK] * 3, [OK] * 3), None)
    bad = blk.copy()
    _tamper_proof(bad, 0)
    s0 = RP.block_seeds(SEED)[0]
    ok, status, _ = nat.verify_batch(bad.coms[:NPROOFS], bad.proofs, s0, want_status=True)
    cb, pb = (np.frombuffer(b"".join(x), dtype=np.uint8) for x in (bad.coms[:NPROOFS], bad.proofs))
    acc, xy, sd = C.c_int(-1), np.zeros(8, dtype=np.uint64), np.frombuffer(s0, dtype=np.uint8)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    assert gpu.lib.bppp_rp_verify_batch(nat.h, NPROOFS, vp(cb), vp(pb), vp(sd), C.byref(acc), None, None, vp(xy)) == 0
    V = array_to_point(xy)
    got = _both(nat, bad)
    assert not ok and V is not None and got == (False, (status, [OK] * 3, [OK] * 3), V)
