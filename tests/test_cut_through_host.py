"""cut_through_host (bulletproofspp_amd/rangeproof.py), the plain restatement of bppp_rp_cut_through that every GPU test of the call compares against,
on hand-made jobs whose answers are written out here, and a property check on seeded random jobs.  Rows are byte strings: the call never lifts a
point, so no curve is needed.  No GPU, no backend."""
import pytest

from bulletproofspp_amd import rangeproof as rp
from cut_through_jobs import A, B, C, D, N, P, hand_made, hand_made_two_ranges, one_identity, random_job, row

KEPT, SPENT, AGAIN = rp.CUT_KEPT, rp.CUT_SPENT, rp.CUT_KEPT_AGAIN
SUBBIT = rp.TALLY_SUBTRACT
JOBS = hand_made()
JOBS2 = hand_made_two_ranges()


def run(j):
    return rp.cut_through_host(j["nranges"], j["rows"], j["sum_start"], j["entries"], j["claims"])


def test_chain_leaves_first_input_and_last_output():
    r = run(JOBS["chain"])
    assert r.entry_status == [KEPT, SPENT, SPENT, SPENT, SPENT, KEPT]
    assert r.row_map == [5, 0] and r.out_rows == 1                      # D, the new output, in front of A
    assert r.coms_files == [row([D]), row([A])]
    assert r.entries == [1 | SUBBIT, 0]                                 # - A + D in job order, re-based
    assert r.counts == dict(new_rows=2, out_rows=1, new_nnz=2, ncut=4, nagain=0) and r.claims is None


def test_add_and_subtract_inside_one_transaction():
    r = run(JOBS["inside_one_tx"])
    assert r.entry_status == [KEPT, SPENT, SPENT] and r.row_map == [0] and r.out_rows == 0 and r.entries == [SUBBIT]


def test_two_equal_outputs_one_spend():
    r = run(JOBS["two_outputs_one_spend"])
    assert r.entry_status == [SPENT, KEPT, SPENT] and r.row_map == [1] and r.out_rows == 1 and r.entries == [0]


def test_three_equal_outputs_one_spend():
    r = run(JOBS["three_outputs_one_spend"])
    assert r.entry_status == [SPENT, KEPT, AGAIN, SPENT] and r.row_map == [1, 2] and r.entries == [0, 1] and r.counts["nagain"] == 1


def test_double_spend_is_marked():
    r = run(JOBS["double_spend"])
    assert r.entry_status == [KEPT, KEPT, AGAIN] and r.row_map == [2, 0, 1] and r.out_rows == 1
    assert r.entries == [1 | SUBBIT, 0, 2 | SUBBIT]


def test_x_matches_x_plus_p():
    r = run(JOBS["x_plus_p"])
    assert r.entry_status == [SPENT, SPENT] and r.row_map == [] and r.entries == [] and r.counts["ncut"] == 2


def test_sign_bit_is_part_of_the_identity():
    r = run(JOBS["sign_differs"])
    assert r.entry_status == [KEPT, KEPT] and r.row_map == [0, 1] and r.out_rows == 1


def test_padding_bits_are_not():
    assert run(JOBS["padding_differs"]).entry_status == [SPENT, SPENT]


def test_same_flat_index_with_both_signs():
    r = run(JOBS["same_index_both_signs"])
    assert r.entry_status == [SPENT, KEPT, SPENT] and r.row_map == [1] and r.entries == [0]


def test_row_order_outputs_first_each_group_ascending():
    r = run(JOBS["row_order"])
    assert r.row_map == [1, 3, 0, 2] and r.out_rows == 2 and r.entries == [2 | SUBBIT, 0, 3 | SUBBIT, 1]
    r = run(JOBS["mixed_counts"])
    assert r.entry_status == [KEPT, KEPT, SPENT, SPENT, SPENT, KEPT, SPENT]
    assert r.row_map == [0, 2, 4] and r.out_rows == 1 and r.entries == [1 | SUBBIT, 0, 2 | SUBBIT]


def test_half_spent_two_range_rows_stay_whole():
    r = run(JOBS2["half_spent_output"])
    assert r.entry_status == [KEPT, SPENT, SPENT] and r.row_map == [0] and r.out_rows == 1 and r.entries == [0]
    assert r.coms_files == [JOBS2["half_spent_output"]["rows"][0]]      # both ranges, byte for byte
    r = run(JOBS2["half_spent_input"])
    assert r.entry_status == [KEPT, SPENT, SPENT, KEPT]
    assert r.row_map == [1, 0] and r.out_rows == 1                      # row 1 keeps its added D; row 0 survives for - A only: not an output
    assert r.entries == [2 | SUBBIT, 0]


def test_signs_per_range_pairs_by_bit():
    """row 0 = (A sign 1, A sign 0) added, row 1 = (A sign 0, A sign 1) subtracted: entry 0 pairs with entry 3, entry 1 with entry 2"""
    j = JOBS2["signs_per_range"]
    assert rp.cut_identity(2, j["rows"][0], 0) == rp.cut_identity(2, j["rows"][1], 1) == (A, 1)
    assert rp.cut_identity(2, j["rows"][0], 1) == rp.cut_identity(2, j["rows"][1], 0) == (A, 0)
    r = run(j)
    assert r.entry_status == [SPENT] * 4 and r.row_map == [] and r.counts["ncut"] == 4


def test_claims_are_summed_mod_n():
    r = run(JOBS["claims"])
    assert r.claims == ((-5) % N, (3 + N - 1) % N, (N - 2 + 5) % N) and r.row_map == [3, 0]
    assert run(JOBS["claims_wrap"]).claims == (N - 2, 0, 1)
    two = dict(JOBS["claims"], claims=[(-7, N - 2), (2, 5)])                # the binary handle's shape
    assert run(two).claims == ((-5) % N, 3)
    with pytest.raises(ValueError, match="sum 1"):
        run(dict(JOBS["claims"], claims=[(0, 0, 0), (0, N, 0)]))


def test_empty_jobs():
    zero = dict(new_rows=0, out_rows=0, new_nnz=0, ncut=0, nagain=0)
    for r in (rp.cut_through_host(1, [], [0], []), rp.cut_through_host(1, [row([A])], [0, 0, 0], [], [(1, 2, 3), (4, 5, 6)])):
        assert r.counts == zero and r.entries == [] and r.row_map == [] and r.coms_files == [] and r.entry_status == []
    assert rp.cut_through_host(1, [row([A])], [0, 0], [], [(1, 2, 3)]).claims == (0, 0, 0)


def test_bad_arrays_are_refused():
    with pytest.raises(ValueError):
        rp.cut_through_host(1, [row([A])], [0, 2], [0])
    with pytest.raises(ValueError):
        rp.cut_through_host(1, [row([A])], [0, 1], [1])


def test_one_identity_jobs():
    r = run(one_identity(1000, alternate=True))
    assert r.counts == dict(new_rows=0, out_rows=0, new_nnz=0, ncut=1000, nagain=0)
    r = run(one_identity(1000, alternate=False))
    assert r.entry_status == [KEPT] + [AGAIN] * 999 and r.row_map == [0, 1] and r.out_rows == 2


@pytest.mark.parametrize("nranges", [1, 2])
def test_random_jobs_keep_every_net_count(nranges):
    """per identity: (surviving added) - (surviving subtracted) = (added) - (subtracted), no identity survives with both signs, the kept-again marks
    are exactly the survivors behind the first, and the new pool holds the bytes the surviving entries referenced"""
    for seed in range(150):
        j = random_job(seed, 1 + (seed * 7) % 120, nranges)
        r = run(j)
        nr = j["nranges"]
        ident = lambda files, e: rp.cut_identity(nr, files[(e & (SUBBIT - 1)) // nr], (e & (SUBBIT - 1)) % nr)
        before, after = {}, {}
        for e in j["entries"]:
            before.setdefault(ident(j["rows"], e), [0, 0])[e >> 31] += 1
        for e in r.entries:
            after.setdefault(ident(r.coms_files, e), [0, 0])[e >> 31] += 1
        for idt, (p, m) in before.items():
            sp, sm = after.get(idt, [0, 0])
            assert sp - sm == p - m and not (sp and sm), (seed, idt)
        assert set(after) <= set(before)
        kept = [(e, s) for e, s in zip(j["entries"], r.entry_status) if s != SPENT]
        assert [ident(j["rows"], e) for e, _ in kept] == [ident(r.coms_files, e) for e in r.entries]
        assert [e >> 31 for e, _ in kept] == [e >> 31 for e in r.entries]
        seen = set()
        for e, s in kept:
            assert (s == AGAIN) == (ident(j["rows"], e) in seen), seed
            seen.add(ident(j["rows"], e))
        outs = r.row_map[:r.out_rows]
        assert outs == sorted(outs) and r.row_map[r.out_rows:] == sorted(r.row_map[r.out_rows:]) and len(set(r.row_map)) == len(r.row_map)
        assert set(outs) == {(e & (SUBBIT - 1)) // nr for e, _ in kept if not e >> 31}
        assert r.counts["ncut"] + r.counts["new_nnz"] == len(j["entries"]) and r.counts["ncut"] % 2 == 0
        assert r.claims == tuple(sum(c[k] for c in j["claims"]) % N for k in range(3))
