"""The seeded schema sweep (tests/schema_sweep.py) on the CPU: what the generated list covers, that the host protocol code
(bulletproofspp_amd/rangeproof.py, rangeproof_binary.py over the oracle backend) proves and verifies every witness of every member, and
the quirks of the reference's makeRangeData that decide which schemas the sweep may contain.

The quirk: for a reciprocal range of width w = max - min with 2 <= w < base, makeRangeData (TypedReciprocal.hs:103-120) takes its third
branch and gives the leading coefficient w - base < 0 beside a coefficient 1 under a digit of radix base — the digits then bound
value - min by base, not by w.  The native layer refuses such a range (csrc/rpsetup.hpp make_range_data); the Python restatement stays the
reference's formula, and this file pins exactly which (base, w) are affected."""
import pytest

import pyoracle as O
import schema_sweep as SW
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from test_few_rounds_host import PointBackend

N = O.N


def _setups():
    return [(s, SW.host_setup(RP.Backend(), s)) for s in SW.sweep()]


def _live(s):
    """(range, range data) of the reciprocal ranges that are not assumed"""
    return [(r, rd) for r, rd in zip(s.ranges, SW.range_data(s)) if not r[5]]


def test_the_sweep_is_deterministic_and_within_its_limits():
    a, b = SW.sweep(), SW.sweep()
    assert [s.name for s in a] == [s.name for s in b] and a == b
    rec, bins = [s for s in a if not s.binary], [s for s in a if s.binary]
    assert len(rec) == SW.N_RECIPROCAL == 32 and len(bins) == SW.N_BINARY == 12
    for kind in (rec, bins):
        assert {s.flavour for s in kind} == {"NL", "IP"} and abs(sum(s.flavour == "NL" for s in kind) - len(kind) / 2) <= len(kind) / 4
    dropped, candidates = SW.discarded()
    print("discarded %d of %d candidates" % (dropped, candidates))
    assert candidates == len(a) + dropped and 4 * dropped <= candidates
    over = []
    for s, st in _setups():
        assert len(s.wits) == 3 and all(len(w) == len(s.ranges) for w in s.wits)
        if st.nrm_len > SW.MAX_NRM:
            over.append(s)
        assert st.lin_len <= SW.MAX_LIN
        if s.binary:
            assert s.cons
            continue
        for (base, lo, hi, shared, _, assumed), rd in zip(s.ranges, SW.range_data(s)):
            assert hi - lo >= base                                 # nothing the library refuses as narrower than its base
            assert s.cons or not assumed                           # assumed ranges only under types
            if not shared and not assumed:                         # the rule of csrc/rpsetup.hpp make_setup
                assert len(rd.base_coeffs) >= (1 if rd.has_bit else 0) + base - 1
    # the one member above the norm limit: the binary range of width 2^64, alone
    assert [(s.binary, len(s.ranges), s.ranges[0][1] - s.ranges[0][0]) for s in over] == [(True, 1, 2**64)]


def test_the_sweep_covers_what_it_claims():
    setups = _setups()
    rec = [(s, st) for s, st in setups if not s.binary]
    bins = [(s, st) for s, st in setups if s.binary]
    # each coefficient form, as a shared and as an inline range
    seen = {(SW.form_of(r[0], r[2] - r[1]), r[3]) for s, _ in rec for r, _ in _live(s)}
    assert seen == {(f, sh) for f in SW.FORMS for sh in (False, True)}
    for s, _ in rec:                                               # the forms are what make_range_data makes of them
        for r, rd in _live(s):
            form, w, n1 = SW.form_of(r[0], r[2] - r[1]), r[2] - r[1], RP.integer_log(r[0], r[2] - r[1] - 1)
            assert rd.has_bit == form.startswith("bit") and len(rd.base_coeffs) == SW.digit_count(form, n1)
            assert (form == "power") == (w == r[0] ** len(rd.base_coeffs) and not rd.has_bit)
            assert (form == "bit") == (rd.has_bit and w < 2 * r[0] ** n1)
    # an inline range whose symbols equal its digits exactly
    assert any(not r[3] and len(rd.base_coeffs) == (1 if rd.has_bit else 0) + r[0] - 1 for s, _ in rec for r, rd in _live(s))
    # a shared base-2 range beside a shared range with a leading bit of another base: 2 enters m_bases from both sides
    assert any(any(r[3] and r[0] == 2 for r, _ in _live(s)) and any(r[3] and r[0] != 2 and rd.has_bit for r, rd in _live(s)) and 2 in st.m_bases
               for s, st in rec)
    nb = {len(st.sorted_bases) for _, st in rec}
    assert {1, 2, 3} <= nb and max(nb) >= 4
    los = [r[1] for s, _ in rec for r in s.ranges]
    assert any(lo == 0 for lo in los) and any(0 < lo < 2**64 for lo in los) and any(lo < 0 for lo in los) and any(lo >= 2**64 for lo in los)
    assert {r[4] for s, _ in rec for r in s.ranges} == {False, True}                     # outputs and inputs
    assert any(r[5] for s, _ in rec for r in s.ranges)                                   # an assumed range
    assert {s.cons for s, _ in rec} == {False, True}
    lens = {len(s.pubs) for s, _ in rec if s.cons}
    assert {0, 1} <= lens and max(lens) >= 3
    for s, _ in rec:
        if len(s.pubs) >= 3:                                       # an input, an output and a pair that cancels
            assert {io for io, _, _ in s.pubs} == {False, True}
            assert any(a[0] != b[0] and a[1:] == b[1:] for a in s.pubs for b in s.pubs)
        assert s.cons or not s.pubs
    assert any(len(s.pubs) >= 3 and len({ty for _, ty, _ in s.pubs}) == 2 for s, _ in rec)        # the pair in a type of its own
    for kind in (rec, bins):
        assert {s.flavour for s, _ in kind} == {"NL", "IP"}
    assert {st.nrm_len % 4 for _, st in rec} == {0, 1, 2, 3} and {st.lin_len % 4 for _, st in rec} == {0, 1, 2, 3}
    assert len({st.rounds for _, st in rec}) >= 3
    # what the three-kernel test of the GPU file picks from
    assert any(s.cons and any(r[5] for r in s.ranges) for s, _ in rec) and any(not s.cons and len(st.sorted_bases) >= 3 for s, st in rec)
    # binary setups
    ws = [hi - lo for s, _ in bins for lo, hi, _, _ in s.ranges]
    assert {1, 2, 3, 2**64} <= set(ws)
    assert any(w > 2 and w & (w - 1) == 0 and w < 2**64 for w in ws) and any(w > 3 and (w - 1) & (w - 2) == 0 for w in ws)
    assert any(lo < 0 for s, _ in bins for lo, _, _, _ in s.ranges) and any(asm for s, _ in bins for _, _, _, asm in s.ranges)
    assert {len(s.pubs) for s, _ in bins} == {0, 1}
    assert len({st.rounds for _, st in bins}) >= 3


def test_witnesses_sit_where_they_claim():
    """the first row at the minima, the second at max - 1: every range of an untyped setup, as far as the balance allows in a balanced one;
    every amount of a live range in its range, every balanced row balanced"""
    for s in SW.sweep():
        rows = SW._rows_of(s.ranges, s.binary)
        for k, wit in enumerate(s.wits):
            for (sg, lo, hi1, assumed), v in zip(rows, wit):
                assert assumed or lo <= v <= hi1
            if s.cons:
                assert s.net_public + sum(sg * v for (sg, _, _, _), v in zip(rows, wit)) == 0
            if k < 2:
                at_end = [assumed or v == (lo if k == 0 else hi1) for (sg, lo, hi1, assumed), v in zip(rows, wit)]
                assert all(at_end) or s.cons
    # where an assumed range takes the difference, every live range of a typed setup stays at its end
    assert any(all(r[5] or v == r[1] for v, r in zip(s.wits[0], s.ranges)) for s in SW.sweep() if s.cons and not s.binary)


@pytest.mark.parametrize("name", [s.name for s in SW.sweep() + SW.edge_setups()])
def test_honest_proofs_verify(oracle_lib, name):
    s = SW.by_name(name)
    mod = BRP if s.binary else RP
    be = PointBackend(oracle_lib)
    st = SW.host_setup(be, s)
    for j in range(3):
        proof = SW.host_prove(st, s, j)
        assert mod.verify(st, proof, RP.sha256_oracle()) and be.last is None, j
        assert len(proof.responses) == st.rounds and (len(proof.wit_nrm), len(proof.wit_lin)) == tuple(st.final_lens)
        assert not mod.verify(st, proof, RP.sha256_oracle(b"another oracle")) and be.last is not None


# ----------------------------------------------------------------------------- the reference's quirks, pinned
def _top(rd):
    """the largest value the digits can represent"""
    return sum(((2 if (rd.has_bit and i == 0) else rd.base) - 1) * c for i, c in enumerate(rd.base_coeffs))


def test_reciprocal_coefficients_over_a_box_of_bases_and_widths():
    """base 2 .. 17, w 1 .. 2999: the leading coefficient is negative exactly for 2 <= w < base (120 pairs) and zero exactly for w = 1 (16
    pairs); everywhere else the coefficients are positive, the largest representable value is w - 1, and digits recombine"""
    negative, zero = [], []
    for base in range(2, 18):
        for w in range(1, 3000):
            rd = RP.make_range_data(base, 0, w)
            cs = rd.base_coeffs
            if min(cs) < 0:
                negative.append((base, w))
                assert cs == [w - base, 1] and rd.has_bit
                continue
            if min(cs) == 0:
                zero.append((base, w))
                assert cs == [0]
                with pytest.raises(ZeroDivisionError):
                    RP.digits(rd, 0)
                continue
            assert _top(rd) == w - 1, (base, w)
            assert len(cs) == SW.digit_count(SW.form_of(base, w), RP.integer_log(base, w - 1))
            for v in {0, 1 % w, w // 3, w // 2, max(w - 2, 0), w - 1} | ({base - 1, base, cs[0] - 1, cs[0], cs[0] + 1} & set(range(w))):
                ds = RP.digits(rd, v)
                assert sum(d * c for d, c in zip(ds, cs)) == v, (base, w, v)
                assert all(0 <= d < (2 if (rd.has_bit and i == 0) else base) for i, d in enumerate(ds))
    assert negative == [(base, w) for base in range(2, 18) for w in range(2, base)] and len(negative) == 120
    assert zero == [(base, 1) for base in range(2, 18)] and len(zero) == 16
    for base, w in SW.NARROW:                                      # what the GPU file expects bppp_rp_create to refuse
        assert (base, w) in negative
    assert (4, 4) not in negative and (4, 5) not in negative


def test_every_value_of_every_width_in_the_box_recombines():
    """exhaustive: every value 0 .. w - 1 of every accepted (base, w) of the box.  `digits` itself on every value of the widths up to 300; for the
    whole box its greedy rule d = min(radix - 1, n div coeff) on all values of a width at once (numpy), which leaves no remainder exactly
    when the digits recombine; and the reason it does: below every coefficient the remaining digits reach coeff - 1, so no value is skipped"""
    import numpy as np
    for base in range(2, 18):
        for w in range(base, 3000):
            rd = RP.make_range_data(base, 0, w)
            radix = [2 if (rd.has_bit and i == 0) else base for i in range(len(rd.base_coeffs))]
            n = np.arange(w, dtype=np.int64)
            for r, c in zip(radix, rd.base_coeffs):
                n -= np.minimum(r - 1, n // c) * c
            assert not n.any(), (base, w)
            tops = [sum((r - 1) * c for r, c in zip(radix[i:], rd.base_coeffs[i:])) for i in range(len(radix) + 1)]
            assert tops[0] == w - 1 and all(tops[i + 1] >= c - 1 for i, c in enumerate(rd.base_coeffs)), (base, w)
            if w <= 300:
                for v in range(w):
                    assert sum(d * c for d, c in zip(RP.digits(rd, v), rd.base_coeffs)) == v, (base, w, v)


def test_binary_coefficients_bound_every_width():
    for w in range(1, 3000):
        rd = BRP.make_range_data(5, 5 + w)
        assert sum(rd.base_coeffs) == w - 1 and min(rd.base_coeffs) >= 0
        for v in {0, w // 2, w - 1, min(rd.base_coeffs[0], w - 1), min(rd.base_coeffs[0] + 1, w - 1)}:
            ds = BRP.make_digits(rd, 5 + v)
            assert len(ds) == len(rd.base_coeffs) and set(ds) <= {0, 1} and sum(d * c for d, c in zip(ds, rd.base_coeffs)) == v
