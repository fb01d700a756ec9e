"""Arguments of zero and one round on the CPU: the host protocol code (bulletproofspp_amd/rangeproof.py, rangeproof_binary.py) over the
oracle backend, at the smallest setups the library accepts — a flag in [0, 2), two bits, a trit; binary setups of one or two bits.

With k the number of argument rounds: a typed-reciprocal setup of one small range has k = 1 (linLen = 6 alone asks for one halving), a
binary setup of one or two digits has k = 0 (the final opening IS the witness, no response is sent).  Pinned here, before the GPU is
compared with it (tests/test_gpu_few_rounds.py imports the table and the helpers below): the shapes setup gives, that honest proofs
verify, the lengths of what a proof carries, and that every single-field change of the verifier's inputs is rejected.

Binary k = 0 against the reference: its prover takes integerLog 2 nrmLen - 1 rounds (src/RangeProof/Binary.hs:195),
its verifier and decoder optimalWitnessSize.  For nrmLen = 2 both give 0; for nrmLen = 1 the prover's -1 is `replicate (-1) ()` = no
round (src/Bulletproof.hs:358), again 0.  So the reference itself proves and verifies these layouts, and the native layer must handle them
bit-exactly ("Binary setups of zero rounds")."""
import copy
import dataclasses
import random

import pytest

import pyoracle as O
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from rp_backends import OracleBackend

N = O.N
TY = 15                                                            # the type of every typed amount below

# name: (binary, ranges, typed / conserved, {flavour: (nrm_len, lin_len, rounds, final_lens)}, amounts of three witnesses)
# reciprocal ranges: (base, lo, hi, shared, output, assumed); binary ranges: (lo, hi, output, assumed).  The single range of a typed or
# conserved setup is an output balanced by one public input of the same amount; two binary ranges balance each other.
SETUPS = {
    "flag": (False, [(2, 0, 2, False, True, False)], False, {"NL": (1, 6, 1, (1, 3)), "IP": (1, 6, 1, (2, 3))}, [[0], [1], [1]]),
    "flag typed": (False, [(2, 0, 2, False, True, False)], True, {"NL": (2, 6, 1, (1, 3)), "IP": (2, 6, 1, (2, 3))}, [[1], [0], [1]]),
    "two bits typed": (False, [(2, 0, 4, False, True, False)], True, {"NL": (3, 6, 1, (2, 3)), "IP": (3, 6, 1, (2, 3))}, [[2], [0], [3]]),
    "shared flag": (False, [(2, 0, 2, True, True, False)], False, {"NL": (1, 7, 1, (1, 4)), "IP": (1, 7, 2, (2, 2))}, [[1], [0], [1]]),
    "shared trit": (False, [(3, 0, 3, True, True, False)], False, {"NL": (1, 8, 1, (1, 4)), "IP": (1, 8, 2, (2, 2))}, [[1], [0], [2]]),
    "binary bit": (True, [(0, 2, True, False)], True, {"NL": (1, 2, 0, (1, 2))}, [[1], [0], [1]]),
    "binary two bits": (True, [(0, 4, True, False)], True, {"NL": (2, 2, 0, (2, 2))}, [[2], [0], [3]]),
    "binary 2 x bit": (True, [(0, 2, True, False), (0, 2, False, False)], True, {"IP": (2, 2, 0, (2, 2))}, [[1, 1], [0, 0], [1, 1]]),
    "binary nibble": (True, [(0, 16, True, False)], True, {"NL": (4, 2, 1, (2, 1))}, [[7], [0], [15]]),
    "binary 2 x two bits": (True, [(0, 4, True, False), (0, 4, False, False)], True, {"IP": (4, 2, 1, (2, 1))}, [[2, 2], [0, 0], [3, 3]]),
}
CASES = [(name, fl) for name, row in SETUPS.items() for fl in row[3]]


def public_amount(name, amounts):
    """the one public amount that balances a proof of these amounts: None for a setup without one"""
    binary, ranges, cons, _, _ = SETUPS[name]
    if not cons or len(ranges) != 1:
        return None
    return amounts[0]


def make_setup(backend, name, flavour, amounts=None):
    """the setup of the table over `backend`; a typed / conserved single-range setup carries the public amount that balances `amounts`
    (default: the first witness of the table)"""
    binary, ranges, cons, _, wits = SETUPS[name]
    pub = public_amount(name, wits[0] if amounts is None else amounts)
    if binary:
        rds = [BRP.make_range_data(*r) for r in ranges]
        pts = O.hash_points(b"few rounds binary", 4 + sum(len(rd.base_coeffs) for rd in rds))
        return BRP.setup(backend, pts, cons, rds, pub or 0, flavour)
    rds = [RP.make_range_data(*r) for r in ranges]
    pts = O.hash_points(b"few rounds", 2 + 8 + 4)
    return RP.setup(backend, pts, cons, [(False, TY, pub)] if cons else [], rds, flavour)


def with_public(st, name, amounts):
    """`st` for a proof of other amounts: the public amount replaced, nothing else"""
    pub = public_amount(name, amounts)
    if pub is None:
        return st
    return dataclasses.replace(st, net_public=pub) if SETUPS[name][0] else dataclasses.replace(st, pub_vt=[(False, TY, pub)])


def inputs_of(name, amounts, seed):
    """the prover's rows for one proof: (amount, blinding) per binary range, (amount, type, blinding) per reciprocal one"""
    rnd = random.Random("few rounds blinding %s %r" % (name, seed))
    binary, _, cons, _, _ = SETUPS[name]
    if binary:
        return [(v, rnd.randrange(N)) for v in amounts]
    return [(v, TY if cons else 0, rnd.randrange(N)) for v in amounts]


def host_prove(st, name, amounts, seed, prefix):
    mod = BRP if SETUPS[name][0] else RP
    st1 = with_public(st, name, amounts)
    return mod.prove(st1, mod.witness(st1, inputs_of(name, amounts, seed)), RP.sha256_oracle(), RP.hash_to_scalar(prefix))


def verifier_inputs(st, binary, proof):
    """what verifyBPM consumes for one proof: RP.verify_inputs, and the same dictionary for a binary setup (BRP.verify's own steps)"""
    if not binary:
        return RP.verify_inputs(st, proof, RP.sha256_oracle())
    if len(proof.responses) != st.rounds or (len(proof.wit_nrm), len(proof.wit_lin)) != st.final_lens or len(proof.coms) != 2 + len(st.rds):
        return None
    tr = RP.Transcript(RP.sha256_oracle())
    sbp = BRP.verify_rp(st, proof.coms, tr)
    es = []
    for a, b in reversed(proof.responses):
        es.insert(0, tr.oracle([a, b], 1)[0])
    pad = lambda xs, n: list(xs) + [0] * (n - len(xs))
    return {"q": sbp.q, "sp": sbp.pub.sc, "pub_norm": pad(sbp.pub.nrm, st.nrm_len), "pub_lin_c": list(sbp.cs), "pub_lin_x": [0, 0], "es": es,
            "responses": list(proof.responses), "wit_norm": list(proof.wit_nrm), "wit_lin": list(proof.wit_lin), "init_terms": sbp.init_terms}


# ----------------------------------------------------------------------------- the verifier's point on the CPU oracle
def oracle_point(ec, flavour, g, gs, hs, v):
    """E = commit(the term list verifyBPM builds) for the verifier inputs `v` (OracleBackend.verify_bp's calls): None iff the proof verifies"""
    nl, ll = len(gs), len(hs)
    pad = lambda xs, n: list(xs) + [0] * (n - len(xs))
    if flavour == "NL":
        basis = O.PSV(0, g, O.NormLinear.make(1, v["q"], [0] * ll, [0] * nl, gs, [0] * ll, hs))
        pub = O.PSV(v["sp"] % N, g, O.NormLinear.make(1, v["q"], pad(v["pub_lin_c"], ll), pad(v["pub_norm"], nl), [None] * nl, pad(v["pub_lin_x"], ll), [None] * ll))
        witb = O.NormLinear.make(1, 1, [], v["wit_norm"], [], v["wit_lin"], [])
        return O.commit(O.verify_terms(v["init_terms"], v["es"], v["responses"], pub, basis, witb), ec)
    basis = O.PSV(0, g, O.NormLinearIP.make(1, v["q"], [0] * ll, [0] * nl, gs, [0] * ll, hs, ec))
    pub = O.PSV(v["sp"] % N, g, O.NormLinearIP.make(1, v["q"], pad(v["pub_lin_c"], ll), pad(v["pub_norm"], nl), [None] * nl, pad(v["pub_lin_x"], ll), [None] * ll, ec))
    witb = O.NormLinearIP.make(1, 1, [], v["wit_norm"], [], v["wit_lin"], [], ec)
    return O.commit(O.verify_terms_generic(O.NormLinearIP, v["init_terms"], v["es"], v["responses"], pub, basis, witb), ec)


class PointBackend(OracleBackend):
    """the oracle backend whose verifier also hands back the committed point (`last`)"""

    def verify_bp(self, flavour, q, sp, g, pub_nrm, gs, cs, pub_lin, hs, es, responses, wit_nrm, wit_lin, init_terms):
        self.last = oracle_point(self.ec, flavour, g, gs, hs, {"q": q, "sp": sp, "pub_norm": pub_nrm, "pub_lin_c": cs, "pub_lin_x": pub_lin, "es": es,
                                                               "responses": responses, "wit_norm": wit_nrm, "wit_lin": wit_lin, "init_terms": init_terms})
        return self.last is None


# ----------------------------------------------------------------------------- single-place changes of the verifier's inputs
def changes(ec, v, nl):
    """[(place, changed copy of v)]: every place of the verifier's inputs changed alone.  Scalars stay canonical, challenges non-zero and
    points on the curve.  Places that cannot exist at a shape are left out: no final norm scalar and no last entry of pub_norm without a
    norm vector (nl = 0), where q / r enters nothing either (it only weighs norm positions); no linear place without a linear vector; no
    response at k = 0."""
    out = []

    def put(place, key, idx, new):
        w = copy.deepcopy(v)
        if idx is None:
            w[key] = new
        else:
            w[key][idx] = new
        out.append((place, w))

    for i, s in enumerate(v["wit_norm"]):
        put("final norm %d" % i, "wit_norm", i, (s + 1) % N)
    for i, s in enumerate(v["wit_lin"]):
        put("final lin %d" % i, "wit_lin", i, (s + 1) % N)
    for i, e in enumerate(v["es"]):
        put("challenge %d" % i, "es", i, (e + 1) % N or 1)
    if nl:
        put("q", "q", None, (v["q"] + 1) % N or 1)
    put("sp", "sp", None, (v["sp"] + 1) % N)
    for key in ("pub_norm", "pub_lin_x", "pub_lin_c"):
        if v[key]:
            put("last " + key, key, len(v[key]) - 1, (v[key][-1] + 1) % N)
    s0, p0 = v["init_terms"][-1]
    put("init scalar", "init_terms", len(v["init_terms"]) - 1, ((s0 + 1) % N, p0))
    put("init point", "init_terms", len(v["init_terms"]) - 1, (s0, ec.add(p0, p0)))
    k = len(v["responses"])
    if k:
        x, r = v["responses"][k - 1]
        put("response pair swapped", "responses", k - 1, (r, x))
        put("response negated", "responses", 0, (v["responses"][0][0], O.PyEC.neg(v["responses"][0][1])))
    if k > 1:
        w = copy.deepcopy(v)
        w["responses"][0], w["responses"][1] = w["responses"][1], w["responses"][0]
        out.append(("two rounds' responses swapped", w))
    return out


PLACES_ALWAYS = {"sp", "init scalar", "init point"}


def places_expected(nl, ll, k, fn, fl):
    want = set(PLACES_ALWAYS) | {"final norm %d" % i for i in range(fn)} | {"final lin %d" % i for i in range(fl)} | {"challenge %d" % i for i in range(k)}
    want |= ({"q", "last pub_norm"} if nl else set()) | ({"last pub_lin_x", "last pub_lin_c"} if ll else set())
    want |= ({"response pair swapped", "response negated"} if k else set()) | ({"two rounds' responses swapped"} if k > 1 else set())
    return want


# ----------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name,flavour", CASES)
def test_shapes_of_the_small_setups(name, flavour):
    """setup alone (no curve arithmetic): the shapes computed for the issue, and k < 2 in all but the two shared inner-product setups"""
    st = make_setup(RP.Backend(), name, flavour)
    want = SETUPS[name][3][flavour]
    assert (st.nrm_len, st.lin_len, st.rounds, tuple(st.final_lens)) == want
    if SETUPS[name][0]:                                            # the reference's binary prover takes the same number of rounds (Binary.hs:195)
        assert max(RP.integer_log(2, st.nrm_len) - 1, 0) == st.rounds


@pytest.mark.parametrize("name,flavour", CASES)
def test_honest_proofs_verify_and_every_change_is_rejected(oracle_lib, name, flavour):
    binary, _, _, shapes, wits = SETUPS[name]
    mod = BRP if binary else RP
    be = PointBackend(oracle_lib)
    st = make_setup(be, name, flavour)
    nrm, lin, k, (fn, fl) = shapes[flavour]
    seen = set()
    for j, amounts in enumerate(wits):                             # every amount at an end of its range included
        st1 = with_public(st, name, amounts)
        proof = host_prove(st, name, amounts, j, b"few rounds host %d" % j)
        assert mod.verify(st1, proof, RP.sha256_oracle()) and be.last is None
        assert len(proof.responses) == k and (len(proof.wit_nrm), len(proof.wit_lin)) == (fn, fl)
        assert len(proof.coms) == (2 if binary else 4) + len(st.rds)
        v = verifier_inputs(st1, binary, proof)
        assert len(v["es"]) == k and len(v["pub_norm"]) == nrm and len(v["pub_lin_c"]) == lin and len(v["pub_lin_x"]) == lin
        assert oracle_point(oracle_lib, flavour, st.g, st.gs, st.hs, v) is None
        for place, w in changes(oracle_lib, v, nrm):
            seen.add(place)
            ok = be.verify_bp(flavour, w["q"], w["sp"], st.g, w["pub_norm"], st.gs, w["pub_lin_c"], w["pub_lin_x"], st.hs, w["es"], w["responses"], w["wit_norm"],
                              w["wit_lin"], w["init_terms"])
            assert not ok and be.last is not None, (j, place)
        # the proof object's own fields: a witness scalar, the commitments exchanged, another oracle
        for field_, idx in (("wit_nrm", 0), ("wit_lin", -1)):
            bad = copy.deepcopy(proof)
            getattr(bad, field_)[idx] = (getattr(bad, field_)[idx] + 1) % N
            assert not mod.verify(st1, bad, RP.sha256_oracle())
        bad = copy.deepcopy(proof)
        bad.coms[0], bad.coms[1] = bad.coms[1], bad.coms[0]
        assert not mod.verify(st1, bad, RP.sha256_oracle())
        assert not mod.verify(st1, proof, RP.sha256_oracle(b"another oracle"))
        if public_amount(name, amounts) is not None:              # the public amount of another proof
            other = with_public(st, name, [amounts[0] + 1])
            assert not mod.verify(other, proof, RP.sha256_oracle())
    assert seen == places_expected(nrm, lin, k, fn, fl)
