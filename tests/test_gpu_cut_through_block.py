"""The point of bppp_rp_cut_through, with real commitments on a 64bit handle: honest transactions made with commit_batch, tally_claims, excess_keys
and excess_sign are merged by ONE call into the block that the block calls accept.
  honest    T = 64 transactions of one input and two outputs, about a third of the outputs spent inside the set through a copy of their row: after
            cut_through, excess_sums_each over the new pool, the one sum, the summed claim and all keys in one group is OPEN_OK
  points    the one sum's point equals bppp_sum_points of the per-transaction points of the un-cut job — exact invariance: what is cut adds and
            subtracts the same term — and still does with one fee off by one, where both sides are MISMATCH
  block     T = 8 with proofs and bindings: assemble_block, then verify_block accepts; with a surviving output's proof swapped for a cut output's
            it rejects"""
import hashlib
import random

import pytest

import pyoracle as O
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
import test_gpu_prove_device as PD

pytestmark = pytest.mark.gpu

N = O.N
TAG = b"cut-through block test"
AUX = hashlib.sha256(b"cut-through aux").digest()
SEED = hashlib.sha256(b"cut-through seed").digest()
OK, MISMATCH = capi.RP_OPEN_OK, capi.RP_OPEN_MISMATCH
_SETS = {}


@pytest.fixture(scope="module")
def nat(gpu):
    h = RP.NativeRangeProofs(gpu, PD._setup(gpu, "64bit"), oracle_tag=TAG)
    h.set_option("comb_min", 1)
    h.set_option("comb_bits", PD.BITS)
    yield h
    h.close()


def _transactions(nat, T, seed, prove=False):
    """T honest transactions as they arrive.  wit: the distinct commitments' (amount, 0, blinding); rows: the witness each pool row holds (a spend
    inside the set brings a second row of the same witness); the job; per transaction the claim (minus its fee, 0, its offset), its key, message
    and signature; with prove, one proof file and binding per row that creates an output (None elsewhere)."""
    key = (T, seed, prove)
    if key in _SETS:
        return _SETS[key]
    rnd = random.Random("cut-through block %d %d" % (T, seed))
    wit, rows, made, txs, unspent = [], [], [], [], []

    def new_row(w, creates):
        rows.append(w)
        made.append(creates)
        return len(rows) - 1

    for t in range(T):
        if unspent and rnd.random() < 0.67:
            w_in = unspent.pop(rnd.randrange(len(unspent)))           # an output of an earlier transaction of the set, through a row of its own
        else:
            wit.append((rnd.randrange(10**6, 2**40), 0, rnd.randrange(N)))
            w_in = len(wit) - 1
        v = wit[w_in][0]
        fee = rnd.randrange(0, min(1000, v) + 1)
        o1 = rnd.randrange(0, v - fee + 1)
        outs = []
        for amount in (o1, v - fee - o1):
            wit.append((amount, 0, rnd.randrange(N)))
            outs.append(len(wit) - 1)
            unspent.append(len(wit) - 1)
        r_in = new_row(w_in, False)
        txs.append([(r_in, True)] + [(new_row(w, True), False) for w in outs])
    rnd.shuffle(txs)                                                   # arrival order is not creation order: a spend may come first
    ss, en = [0], []
    for tx in txs:
        en += [RP.tally_entry(r, sub) for r, sub in tx]
        ss.append(len(en))
    inputs = [[wit[w]] for w in rows]
    proofs = bindings = None
    if prove:
        need = sorted({w for w, creates in zip(rows, made) if creates})
        bind_of = {w: hashlib.sha256(b"cut-through binding %d" % w).digest() for w in need}
        files_of = dict(zip(need, nat.prove_batch([[wit[w]] for w in need], PD._prefixes(len(need), b"cut-through"), bindings=[bind_of[w] for w in need])))
        files = nat.commit_batch(inputs)
        for r, (w, creates) in enumerate(zip(rows, made)):
            if creates:
                assert files_of[w][0] == files[r]                       # the prover's commitments file is commit_batch's
        proofs = [files_of[w][1] if creates else None for w, creates in zip(rows, made)]
        bindings = [bind_of[w] if creates else None for w, creates in zip(rows, made)]
    else:
        files = nat.commit_batch(inputs)
    sums = nat.tally_claims(inputs, ss, en)                             # (- fee mod N, 0, blinding sum) per transaction
    offsets = [rnd.randrange(N) for _ in range(T)]
    secrets = [(e - o) % N for (_, _, e), o in zip(sums, offsets)]
    claims = [(a, ty, o) for (a, ty, _), o in zip(sums, offsets)]
    msgs = [hashlib.sha256(b"cut-through kernel %d" % t).digest() for t in range(T)]
    out = dict(files=files, ss=ss, en=en, claims=claims, keys=nat.excess_keys(secrets), msgs=msgs, sigs=nat.excess_sign(secrets, msgs, AUX), proofs=proofs,
               bindings=bindings, rows=rows, made=made)
    _SETS[key] = out
    return out


def test_honest_transactions_make_a_block_that_balances(gpu, nat):
    T = 64
    s = _transactions(nat, T, 1)
    assert nat.excess_sums_each(s["files"], s["ss"], s["en"], s["claims"], list(range(T + 1)), s["keys"]) == [OK] * T
    cut = nat.cut_through(s["files"], s["ss"], s["en"], s["claims"])
    want = RP.cut_through_host(1, s["files"], s["ss"], s["en"], s["claims"])
    assert (cut.coms_files, cut.entries, cut.row_map, cut.out_rows, cut.entry_status, cut.claims, cut.counts) == \
           (want.coms_files, want.entries, want.row_map, want.out_rows, want.entry_status, want.claims, want.counts)
    assert T // 2 <= cut.counts["ncut"] // 2 <= T and cut.counts["nagain"] == 0                 # about a third of the 2 T outputs are spent inside the set
    assert cut.counts["new_rows"] == 3 * T - cut.counts["ncut"] and cut.out_rows == 2 * T - cut.counts["ncut"] // 2
    assert nat.excess_sums_each(cut.coms_files, [0, len(cut.entries)], cut.entries, [cut.claims], [0, T], s["keys"]) == [OK]
    # one key left out: the block no longer balances
    assert nat.excess_sums_each(cut.coms_files, [0, len(cut.entries)], cut.entries, [cut.claims], [0, T - 1], s["keys"][:-1]) == [MISMATCH]


@pytest.mark.parametrize("fee_off", [False, True], ids=["honest", "fee_off_by_one"])
def test_the_one_sum_is_the_sum_of_the_transactions_sums(gpu, nat, fee_off):
    T = 64
    s = _transactions(nat, T, 1)
    claims = list(s["claims"])
    if fee_off:
        a, ty, o = claims[5]
        claims[5] = ((a + 1) % N, ty, o)
    st_tx, pts_tx = nat.excess_sums_each(s["files"], s["ss"], s["en"], claims, list(range(T + 1)), s["keys"], want_points=True)
    assert st_tx == [MISMATCH if fee_off and t == 5 else OK for t in range(T)]
    cut = nat.cut_through(s["files"], s["ss"], s["en"], claims)
    st_blk, pts_blk = nat.excess_sums_each(cut.coms_files, [0, len(cut.entries)], cut.entries, [cut.claims], [0, T], s["keys"], want_points=True)
    assert st_blk == [MISMATCH if fee_off else OK]
    assert all(p is not None for p in pts_tx) and pts_blk[0] is not None
    assert gpu.sum_points(capi.points_to_array(pts_tx)) == pts_blk[0]


def test_assemble_block_then_verify_block(gpu, nat):
    T = 8
    s = _transactions(nat, T, 2, prove=True)
    kwargs, cut = nat.assemble_block(s["files"], s["ss"], s["en"], s["claims"], s["keys"], s["msgs"], s["sigs"], proof_files=s["proofs"], bindings=s["bindings"])
    assert cut.counts["ncut"] >= 2 and cut.out_rows == len(kwargs["proof_files"]) > 0 and len(kwargs["coms_files"]) == cut.counts["new_rows"]
    assert kwargs["key_start"] == [0, T] and kwargs["sum_start"] == [0, cut.counts["new_nnz"]]
    accept, statuses, _ = nat.verify_block(**kwargs, seed=SEED, want_status=True)
    assert accept and all(v == 0 for part in statuses for v in part)
    # a surviving output under the proof of an output that was cut
    cut_rows = [e for e, v in zip(s["en"], cut.entry_status) if v == capi.RP_CUT_SPENT and not e & RP.TALLY_SUBTRACT]       # one range: an added entry is its row
    assert cut_rows and s["proofs"][cut_rows[0]] is not None
    bad = dict(kwargs, proof_files=[s["proofs"][cut_rows[0]]] + kwargs["proof_files"][1:])
    accept, statuses, _ = nat.verify_block(**bad, seed=SEED, want_status=True)
    assert not accept and statuses[0][0] != 0
