"""Arguments of zero, one and (as controls) two rounds on the GPU, against the CPU oracle.

With k the number of argument rounds, the verifier's scalar kernels run code of their own for k < 2 (csrc/nlbatch.hip: k_vb_shared1 in place
of k_vb_shared4, the position-by-position branches of k_vb_lin_partial and each_put4), and at k = 0 every `2 * k` stride collapses: no
challenge, no response, a per-proof tail of the init terms alone.  Range proofs of one small range have k = 1, binary ones of one or two
digits k = 0 (tests/test_few_rounds_host.py pins the host side and holds the table of setups and the helpers used here).

 2a. bppp_nl_verify_batch_device / bppp_ip_verify_batch_device over a lattice of shapes (every residue of the lengths mod 4, an empty norm
     vector, an empty linear vector) and batch sizes (1, 2, 5, 33; 70: three tiles a group in k_vb_sum_partials; 1030: two proofs a tile):
     the combined point equals sum_b rho_b E_b with E_b the oracle's commit of verifyBPM's term list, members changed in one place each;
 2b. bppp_nl_verify / bppp_ip_verify leave the oracle's E_b for every such change;
 2c. the refusals of the untrusted-input validation (rho = 0, a scalar = n, a point off the curve or with x >= p; a point fault wins);
 3.  the range-proof layer on the setups of the table: the prover's bytes, verdict and point parity of verify_batch / verify_each on
     every single-field mutation of a proof, a batch of 1030, and a mixed job.

Every comparison is exact; every expected value comes from oracle/pyoracle.py, the C oracle and the host protocol code."""
import json
import os
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import encoding as E
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import _ptr, array_to_point, int_to_limbs, points_to_array, scalars_to_array
from rp_backends import OracleBackend
from test_few_rounds_host import CASES, SETUPS, PointBackend, changes, host_prove, inputs_of, make_setup, oracle_point, places_expected, public_amount
from test_gpu_decode_conformance import Layout, Lift
from test_gpu_verify_each import SEED, _batch_full, _rho
from test_rangeproof import EXAMPLES

pytestmark = pytest.mark.gpu

N, P = O.N, O.P
VALID, INVALID = 0, 1
ERR_ARG, ERR_POINT = -1, -4

# (flavour, nl, ll): k = the rounds optimalWitnessSize gives (asserted in _pool and in test_the_lattice_covers_what_it_claims).  Norm-linear
# (5, 3) was asked for as a two-round control, but 5 -> 3 and 3 -> 2 close in ONE round (3 + 2 <= 5): it stays, at its true k, and (9, 5)
# takes its place among the controls
SHAPES = {
    ("NL", 1, 1): 0, ("NL", 2, 2): 0, ("NL", 3, 2): 0, ("NL", 0, 1): 0, ("NL", 1, 0): 0,
    ("NL", 4, 3): 1, ("NL", 5, 1): 1, ("NL", 7, 2): 1, ("NL", 0, 6): 1, ("NL", 2, 6): 1, ("NL", 3, 6): 1, ("NL", 5, 3): 1,
    ("NL", 9, 5): 2, ("NL", 6, 6): 2,
    ("IP", 1, 1): 0, ("IP", 2, 2): 0, ("IP", 3, 1): 0, ("IP", 2, 0): 0,
    ("IP", 3, 2): 1, ("IP", 4, 3): 1, ("IP", 7, 2): 1, ("IP", 0, 6): 1, ("IP", 2, 6): 1, ("IP", 2, 4): 1,
    ("IP", 5, 3): 2, ("IP", 6, 6): 2,
}
SIZES = (1, 2, 5, 33)
# 70 tiles (NL: one proof a tile up to 1024 proofs) make k_vb_sum_partials' groups three tiles long, 33 two; 1030 is the first norm-linear size with
# two proofs a tile (vb_kt), there with k_vb_shared1
MORE_SIZES = {("NL", 3, 2): (70,), ("NL", 7, 2): (70, 1030), ("IP", 3, 1): (70,), ("IP", 7, 2): (70,)}
REFUSAL_SHAPES = {("NL", 7, 2): 1, ("NL", 17, 5): 3, ("IP", 7, 2): 1, ("IP", 16, 6): 3}
NPROOFS = 3


def _size(flavour, nl, ll):
    return O.optimal_witness_size_nl(nl, ll) if flavour == "NL" else O.optimal_witness_size_ip(nl, ll)


# ----------------------------------------------------------------------------- instances proved by the CPU oracle
class Pool:
    """NPROOFS honest arguments of one shape over one basis, proved by the oracle with exactly k rounds, and their changed copies; the
    oracle's point of every member is computed once"""

    def __init__(self, ec, flavour, nl, ll):
        self.ec, self.flavour, self.nl, self.ll = ec, flavour, nl, ll
        self.k, (self.fn, self.fl) = _size(flavour, nl, ll)
        self.ninit = 1 + (nl + ll) % 2                             # 1 for some shapes, 2 for others
        g, *rest = O.hash_points(b"few rounds %s %d %d" % (flavour.encode(), nl, ll), 1 + nl + ll)
        self.g, self.gs, self.hs = g, rest[:nl], rest[nl:]
        self.raw = []
        self.honest = [self._prove(j) for j in range(NPROOFS)]
        self.changed = [changes(ec, v, nl) for v in self.honest]
        self.points = {}

    def _prove(self, j):
        ec, nl, ll, g, gs, hs = self.ec, self.nl, self.ll, self.g, self.gs, self.hs
        rnd = random.Random("few rounds %s %d %d %d" % (self.flavour, nl, ll, j))
        sc = lambda n: [rnd.randrange(1, N) for _ in range(n)]
        xs, ls, cs, pub_n, pub_l = sc(nl), sc(ll), sc(ll), sc(nl), sc(ll)
        q, sp = rnd.randrange(1, N), rnd.randrange(1, N)
        if self.flavour == "NL":
            body = O.NormLinear.make(1, q, cs, xs, gs, ls, hs)
        else:
            body = O.NormLinearIP.make(1, q, cs, xs, gs, ls, hs, ec)
        wit = O.PSV(body.eval_scalar(), g, body)
        # initCom commits to the hidden part: total - pub on every basis element, and s - sp on g
        hidden = [((x - p) % N, G_) for x, p, G_ in zip(xs, pub_n, gs)] + [((x - p) % N, H_) for x, p, H_ in zip(ls, pub_l, hs)] + [((wit.sc - sp) % N, g)]
        com = O.commit(hidden, ec)
        if self.ninit == 1:
            init = [(1, com)]
        else:                                                      # a 2-term opening: t * (t^-1 C1) + 1 * C2 with C1 + C2 = C
            t = rnd.randrange(1, N)
            c1 = ec.mul(rnd.randrange(1, N), g)
            init = [(t, ec.mul(O.inv_mod(t, N), c1)), (1, ec.add(com, O.PyEC.neg(c1)))]
        fin, resps, es = O.prove_bp(self.k, wit, O.Transcript(O.sha_oracle_fn(b"few rounds %d" % j)), ec)
        if self.flavour == "NL":
            nw, lw = fin.body.norm.get_witness(), fin.body.lin.get_witness()
        else:
            w = fin.body.get_witness()
            n2 = 2 * len(fin.body.norm.body)
            nw, lw = w[:n2], w[n2:]
        assert (len(nw), len(lw), len(resps), len(es)) == (self.fn, self.fl, self.k, self.k)
        self.raw.append((wit.sc, q, cs, xs, ls, fin.sc))            # the prover's start state, and the scalar it must end with
        return {"q": q, "sp": sp, "pub_norm": pub_n, "pub_lin_c": cs, "pub_lin_x": pub_l, "es": es, "responses": resps, "wit_norm": nw, "wit_lin": lw, "init_terms": init}

    def point(self, v):
        if id(v) not in self.points:
            self.points[id(v)] = oracle_point(self.ec, self.flavour, self.g, self.gs, self.hs, v)
        return self.points[id(v)]

    def dims(self):
        return self.nl, self.ll, self.k, self.fn, self.fl, self.ninit


_POOLS = {}


def _pool(ec, key, k_want):
    if key not in _POOLS:
        _POOLS[key] = Pool(ec, *key)
    pool = _POOLS[key]
    assert pool.k == k_want
    for v in pool.honest:
        assert pool.point(v) is None
    return pool


# ----------------------------------------------------------------------------- the library calls
SCALAR_ARRAYS = ["rho", "q", "sp", "pub_norm", "pub_lin_c", "pub_lin_x", "es", "wit_norm", "wit_lin", "init_s"]
POINT_ARRAYS = ["g", "G", "H", "init_p", "resp"]
ORDER = ["g", "G", "H", "rho", "q", "sp", "pub_norm", "pub_lin_c", "pub_lin_x", "es", "wit_norm", "wit_lin", "init_s", "init_p", "resp"]
_ROWS = {}


def _rows(v):
    """the per-proof rows of one member as arrays (made once per member: a large batch repeats a few)"""
    if id(v) not in _ROWS:
        s = lambda xs: scalars_to_array([x % N for x in xs])
        _ROWS[id(v)] = (v, {"q": s([v["q"]]), "sp": s([v["sp"]]), "pub_norm": s(v["pub_norm"]), "pub_lin_c": s(v["pub_lin_c"]), "pub_lin_x": s(v["pub_lin_x"]),
                            "es": s(v["es"]), "wit_norm": s(v["wit_norm"]), "wit_lin": s(v["wit_lin"]), "init_s": s([t for t, _ in v["init_terms"]]),
                            "init_p": points_to_array([p for _, p in v["init_terms"]]), "resp": points_to_array([p for xr in v["responses"] for p in xr])})
    return _ROWS[id(v)][1]


def batch_arrays(pool, members, rhos):
    """the fifteen arrays of bppp_{nl,ip}_verify_batch_device; an array without entries is one unused row (the library takes no NULL for it
    only where its length is non-zero, and reads none of it)"""
    rows = [_rows(v) for v in members]
    arrs = {"g": points_to_array([pool.g]), "G": points_to_array(pool.gs), "H": points_to_array(pool.hs), "rho": scalars_to_array(rhos)}
    for name in ORDER[4:]:
        arrs[name] = np.concatenate([r[name] for r in rows])
    for name, a in arrs.items():
        if a.shape[0] == 0:
            arrs[name] = np.zeros((1, a.shape[1]), dtype=np.uint64)
    return arrs


def run_batch(gpu, pool, batch, arrs):
    nl, ll, k, fn, fl, ninit = pool.dims()
    fn_ = gpu.lib.bppp_nl_verify_batch_device if pool.flavour == "NL" else gpu.lib.bppp_ip_verify_batch_device
    dev = [gpu.to_device(arrs[name]) for name in ORDER]
    out = np.zeros(8, dtype=np.uint64)
    try:
        rc = fn_(gpu.h, batch, nl, ll, k, fn, fl, ninit, *[_ptr(d) for d in dev], _ptr(out))
    finally:
        for d in dev:
            gpu.free(d)
    return rc, array_to_point(out)


def batch_point(gpu, pool, members, rhos):
    rc, pt = run_batch(gpu, pool, len(members), batch_arrays(pool, members, rhos))
    gpu._check(rc, "verify_batch_device")
    return pt


def single_point(gpu, pool, v):
    """the point bppp_nl_verify / bppp_ip_verify leaves for one proof"""
    out = np.zeros(8, dtype=np.uint64)
    opt_s = lambda xs: _ptr(scalars_to_array([x % N for x in xs])) if len(xs) else None
    opt_p = lambda ps: _ptr(points_to_array(ps)) if len(ps) else None
    fn_ = gpu.lib.bppp_nl_verify if pool.flavour == "NL" else gpu.lib.bppp_ip_verify
    rc = fn_(gpu.h, _ptr(int_to_limbs(v["q"])), _ptr(int_to_limbs(v["sp"])), _ptr(points_to_array([pool.g])), opt_s(v["pub_norm"]), opt_p(pool.gs), pool.nl,
             opt_s(v["pub_lin_c"]), opt_s(v["pub_lin_x"]), opt_p(pool.hs), pool.ll, opt_s(v["es"]), len(v["es"]), opt_s(v["wit_norm"]), len(v["wit_norm"]),
             opt_s(v["wit_lin"]), len(v["wit_lin"]), opt_s([t for t, _ in v["init_terms"]]), opt_p([p for _, p in v["init_terms"]]), len(v["init_terms"]),
             opt_p([p for xr in v["responses"] for p in xr]), _ptr(out))
    gpu._check(rc, "verify")
    return array_to_point(out)


def weighted_sum(ec, rhos, points):
    """sum_b rho_b E_b on the oracle; equal points are merged first (a large batch repeats a few members)"""
    acc = {}
    for r, e in zip(rhos, points):
        if e is not None:
            acc[e] = (acc.get(e, 0) + r) % N
    terms = [(r, e) for e, r in acc.items() if r]
    return ec.inner_product(terms) if terms else None


# ----------------------------------------------------------------------------- 2a. the combined point over the lattice
@pytest.mark.parametrize("flavour,nl,ll", list(SHAPES))
def test_batch_point_equals_the_oracles_weighted_sum(gpu, oracle_lib, flavour, nl, ll):
    key = (flavour, nl, ll)
    pool = _pool(oracle_lib, key, SHAPES[key])
    rnd = random.Random("few rounds rho %r" % (key,))
    # walk the places, taking each from the next proof in turn: the changed members of the four small batches already cover every place
    nplaces = len(pool.changed[0])
    assert nplaces <= 27 and all([p for p, _ in c] == [p for p, _ in pool.changed[0]] for c in pool.changed)
    all_changes = [(j, *pool.changed[(i + j) % NPROOFS][i]) for j in range(NPROOFS) for i in range(nplaces)]
    nxt, seen = 0, set()
    batches = [[False], [True]] + [[b % 3 != 0 for b in range(B)] for B in SIZES[1:] + MORE_SIZES.get(key, ())]
    for flags in batches:
        B = len(flags)
        members, honest = [], []
        for b, change in enumerate(flags):
            if change:
                _, place, w = all_changes[nxt % len(all_changes)]
                nxt += 1
                seen.add(place)
                members.append(w)
            else:
                members.append(pool.honest[(b // 3) % NPROOFS])
            honest.append(not change)
        rhos = [rnd.randrange(1, N) for _ in range(B)]
        pts = [pool.point(v) for v in members]
        assert [e is None for e in pts] == honest                  # E_b is the identity exactly for the honest members
        want = weighted_sum(oracle_lib, rhos, pts)
        assert (want is None) == all(honest)
        got = batch_point(gpu, pool, members, rhos)
        assert got == want, (key, B)
    assert seen == places_expected(nl, ll, pool.k, pool.fn, pool.fl)


def test_the_lattice_covers_what_it_claims():
    """no GPU work: every k < 2 at every residue of the lengths mod 4, empty vectors, both numbers of init terms, the stated k"""
    for flavour in ("NL", "IP"):
        for k in (0, 1, 2):
            assert any(f == flavour and kk == k for (f, _, _), kk in SHAPES.items())
        assert {ll % 4 for (f, _, ll), k in SHAPES.items() if f == flavour and k < 2} == {0, 1, 2, 3}
    assert {nl % 4 for (f, nl, _), k in SHAPES.items() if f == "NL" and k < 2} == {0, 1, 2, 3}
    assert any(nl == 0 for _, nl, _ in SHAPES) and any(ll == 0 for _, _, ll in SHAPES)
    for (flavour, nl, ll), k in list(SHAPES.items()) + list(REFUSAL_SHAPES.items()):
        assert _size(flavour, nl, ll)[0] == k
    assert _size("IP", 3, 1)[1][0] == 4
    assert {1 + (nl + ll) % 2 for (_, nl, ll), k in SHAPES.items() if k == 0} == {1, 2}
    assert {1 + (nl + ll) % 2 for (_, nl, ll), k in SHAPES.items() if k == 1} == {1, 2}


# ----------------------------------------------------------------------------- 2b. the single-proof verifiers
@pytest.mark.parametrize("flavour,nl,ll", list(SHAPES))
def test_single_proof_point_equals_the_oracles(gpu, oracle_lib, flavour, nl, ll):
    key = (flavour, nl, ll)
    pool = _pool(oracle_lib, key, SHAPES[key])
    assert single_point(gpu, pool, pool.honest[0]) is None and single_point(gpu, pool, pool.honest[1]) is None
    seen = set()
    for place, w in pool.changed[0]:
        want = pool.point(w)
        assert want is not None, place
        assert single_point(gpu, pool, w) == want, (key, place)
        seen.add(place)
    assert seen == places_expected(nl, ll, pool.k, pool.fn, pool.fl)


# ----------------------------------------------------------------------------- the argument's provers at exactly k rounds
@pytest.mark.parametrize("flavour,nl,ll", list(SHAPES))
def test_argument_provers_take_exactly_k_rounds(gpu, oracle_lib, flavour, nl, ll):
    """bppp_nl_* / bppp_ip_* (one proof) and bppp_nlb_* (the proofs in lockstep) over k rounds — none at k = 0, where getWitness reads the
    start state: responses, challenges, final opening and final scalar equal the oracle's"""
    from bulletproofspp_amd.bulletproof import NormLinearBatch, NormLinearBP, NormLinearIP, proveBPM, proveBPM_batch
    key = (flavour, nl, ll)
    pool = _pool(oracle_lib, key, SHAPES[key])
    oracles = [O.Transcript(O.sha_oracle_fn(b"few rounds %d" % j)).oracle for j in range(NPROOFS)]
    for j, (s, q, cs, xs, ls, s_fin) in enumerate(pool.raw):
        v = pool.honest[j]
        if flavour == "NL":
            com = NormLinearBP(gpu, s, pool.g, q, cs, xs, pool.gs, ls, pool.hs)
            resps, es = proveBPM(pool.k, com, oracles[j])
            got = com.getWitness() + (com.download()["s"],)
        else:
            com = NormLinearIP(gpu, s, pool.g, q, cs, xs, pool.gs, ls, pool.hs)
            resps, es = [], []
            for _ in range(pool.k):
                _, lc, _, rc = com.makeScalarsComs()
                e = oracles[j]([lc, rc])
                com.collapse(e)
                resps.insert(0, (lc, rc)); es.insert(0, e)
            got = com.getWitness()
        com.close()
        assert (resps, es) == (v["responses"], v["es"]), j
        assert tuple(got) == (v["wit_norm"], v["wit_lin"], s_fin), j
    if flavour == "NL":
        raw = pool.raw
        com = NormLinearBatch(gpu, [r[0] for r in raw], pool.g, [r[1] for r in raw], [r[2] for r in raw], [r[3] for r in raw], pool.gs, [r[4] for r in raw], pool.hs)
        fresh = [O.Transcript(O.sha_oracle_fn(b"few rounds %d" % j)).oracle for j in range(NPROOFS)]
        resps, es = proveBPM_batch(pool.k, com, fresh)
        nws, lws, s_fins = com.getWitness()
        com.close()
        for j, v in enumerate(pool.honest):
            assert (resps[j], es[j], nws[j], lws[j], s_fins[j]) == (v["responses"], v["es"], v["wit_norm"], v["wit_lin"], raw[j][5]), j


# ----------------------------------------------------------------------------- 2c. refusals
def _expect(gpu, rc, code, text):
    assert rc == code, (rc, gpu.lib.bppp_last_error(gpu.h).decode())
    assert text in gpu.lib.bppp_last_error(gpu.h).decode()


@pytest.mark.parametrize("flavour,nl,ll", list(REFUSAL_SHAPES))
def test_untrusted_inputs_are_refused(gpu, oracle_lib, flavour, nl, ll):
    """Each call is an otherwise honest batch of 3.  None of these inputs can take a kernel out of bounds: the validation kernels only read
    and flag, no index anywhere depends on a scalar's or a point's value, every derived scalar passes through a modular product before the MSM
    sees it, and the points only enter field arithmetic."""
    key = (flavour, nl, ll)
    pool = _pool(oracle_lib, key, REFUSAL_SHAPES[key])
    rnd = random.Random("few rounds refusals %r" % (key,))
    rhos = [rnd.randrange(1, N) for _ in range(3)]
    fresh = lambda: {name: a.copy() for name, a in batch_arrays(pool, pool.honest, rhos).items()}
    rc, pt = run_batch(gpu, pool, 3, fresh())
    assert rc == 0 and pt is None
    a = fresh(); a["rho"][1] = 0
    _expect(gpu, run_batch(gpu, pool, 3, a)[0], ERR_ARG, "rho is zero")
    for name in SCALAR_ARRAYS:
        a = fresh()
        assert a[name].shape[0] >= 3                               # a real entry of every array at these shapes, not the unused row
        a[name][a[name].shape[0] - 2] = int_to_limbs(N)
        _expect(gpu, run_batch(gpu, pool, 3, a)[0], ERR_ARG, "not canonical")
    x_big = next(x for x in range(1, 2**32 + 977) if oracle_lib.lift_x(x) is not None)       # x + p still fits 256 bits
    for name in POINT_ARRAYS:
        for kind in ("off the curve", "x >= p"):
            a = fresh()
            row = a[name].shape[0] - 1
            x, y = array_to_point(a[name][row])
            bad = (x, (y + 1) % P) if kind == "off the curve" else (x_big + P, oracle_lib.lift_x(x_big)[1])
            a[name][row] = points_to_array([bad])[0]
            _expect(gpu, run_batch(gpu, pool, 3, a)[0], ERR_POINT, "not on the curve")
    a = fresh()                                                    # a point fault and a scalar fault together: the point fault is reported
    x, y = array_to_point(a["resp"][0])
    a["resp"][0] = points_to_array([(x, (y + 1) % P)])[0]
    a["wit_lin"][0] = int_to_limbs(N)
    _expect(gpu, run_batch(gpu, pool, 3, a)[0], ERR_POINT, "not on the curve")
    a = fresh(); a["resp"][1] = 0                                  # the infinity encoding of a response is a point: no refusal, the proof just fails
    rc, pt = run_batch(gpu, pool, 3, a)
    assert rc == 0 and pt is not None
    members = [dict(pool.honest[0]), pool.honest[1], pool.honest[2]]
    members[0]["responses"] = [(members[0]["responses"][0][0], None)] + list(members[0]["responses"][1:])
    assert pt == weighted_sum(oracle_lib, rhos, [oracle_point(oracle_lib, flavour, pool.g, pool.gs, pool.hs, m) for m in members])
    rc, pt = run_batch(gpu, pool, 3, fresh())                      # the context still verifies after the refusals
    assert rc == 0 and pt is None


# ----------------------------------------------------------------------------- 3. range proofs of the small setups
def _native(gpu, ec, name, flavour):
    binary = SETUPS[name][0]
    st = make_setup(PointBackend(ec), name, flavour)
    return st, (BRP.NativeBinaryRangeProofs if binary else RP.NativeRangeProofs)(gpu, st), binary


def _publics(name, wits):
    """prove_batch's per-proof public amounts: a list per proof on a typed handle, an int per proof on a binary one, None without any"""
    if public_amount(name, wits[0]) is None:
        return None
    return [public_amount(name, w) for w in wits] if SETUPS[name][0] else [[public_amount(name, w)] for w in wits]


@pytest.mark.parametrize("name,flavour", CASES)
def test_prover_writes_the_host_protocols_bytes(gpu, oracle_lib, name, flavour):
    st, nat, binary = _native(gpu, oracle_lib, name, flavour)
    try:
        shape = SETUPS[name][3][flavour]
        assert (nat.shape["norm_len"], nat.shape["lin_len"], nat.shape["rounds"], (nat.shape["final_norm"], nat.shape["final_lin"])) == shape
        wits = SETUPS[name][4]
        prefixes = [b"few rounds prover %d" % j for j in range(len(wits))]
        inputs = [inputs_of(name, w, j) for j, w in enumerate(wits)]
        want = [E.encode_proof(2 if binary else 4, host_prove(st, name, w, j, prefixes[j])) for j, w in enumerate(wits)]
        pubs = _publics(name, wits)
        assert nat.prove_batch(inputs, prefixes, public_amounts=pubs) == want
        # the device-resident route over a comb table of the basis, hashing on the device and on the host cores, then the host-algebra route
        nat.set_option("comb_min", 1); nat.set_option("comb_bits", 7)
        for host_oracle_max in (0, 2**64 - 1):
            nat.set_option("host_oracle_max", host_oracle_max)
            assert nat.prove_batch(inputs, prefixes, public_amounts=pubs) == want, host_oracle_max
        nat.set_option("host_algebra", 1)
        assert nat.prove_batch(inputs, prefixes, public_amounts=pubs) == want
        nat.set_option("host_algebra", 0)
        ok, status, _ = nat.verify_batch([c for c, _ in want], [p for _, p in want], SEED, want_status=True, public_amounts=pubs)
        assert ok and status == [VALID] * len(wits)
    finally:
        nat.close()


def _mutants(L, cf, pf):
    """[(what, commitments file, proof file)]: each scalar + 1 mod n, each point's sign bit, two points of the proof file exchanged"""
    out = []

    def put(data, off, new):
        d = bytearray(data); d[off:off + len(new)] = new
        return bytes(d)

    def flip(data, off, i):
        d = bytearray(data); d[off + (i >> 3)] ^= 1 << (i & 7)
        return bytes(d)

    def swap(data, i, j):
        d = bytearray(data)
        xi, xj = data[L.p_xs + 32 * i:L.p_xs + 32 * i + 32], data[L.p_xs + 32 * j:L.p_xs + 32 * j + 32]
        d[L.p_xs + 32 * i:L.p_xs + 32 * i + 32], d[L.p_xs + 32 * j:L.p_xs + 32 * j + 32] = xj, xi
        bi, bj = (data[L.p_signs + (i >> 3)] >> (i & 7)) & 1, (data[L.p_signs + (j >> 3)] >> (j & 7)) & 1
        if bi != bj:
            d[L.p_signs + (i >> 3)] ^= 1 << (i & 7); d[L.p_signs + (j >> 3)] ^= 1 << (j & 7)
        return bytes(d)

    for i in range(L.ns):
        v = (E.get_field(pf[32 * i:32 * i + 32], N) + 1) % N
        out.append(("scalar %d" % i, cf, put(pf, 32 * i, E.put_field(v))))
    for i in range(L.npp):
        out.append(("sign of proof point %d" % i, cf, flip(pf, L.p_signs, i)))
    for i in range(L.nr):
        out.append(("sign of input commitment %d" % i, flip(cf, L.c_signs, i), pf))
    out.append(("points 0 and 1 exchanged", cf, swap(pf, 0, 1)))
    out.append(("the last two points exchanged", cf, swap(pf, L.npp - 2, L.npp - 1)))
    assert all((c, p) != (cf, pf) for _, c, p in out)
    return out


@pytest.mark.parametrize("name,flavour", CASES)
def test_verdicts_and_points_on_single_field_mutations(gpu, oracle_lib, name, flavour):
    st, nat, binary = _native(gpu, oracle_lib, name, flavour)
    try:
        nrp = 2 if binary else 4
        L = Layout(nat.shape, nrp)
        lift = Lift(oracle_lib)
        mod = BRP if binary else RP
        cf, pf = E.encode_proof(nrp, host_prove(st, name, SETUPS[name][4][0], 0, b"few rounds parity"))
        ms = _mutants(L, cf, pf)
        files = [("honest", cf, pf)] + ms
        want_ok, want_pts = [], []
        for _, c, p in files:                                      # the host protocol verifier over the CPU oracle, and the point it commits
            coms = E.decode_commitments(L.nr, c, lift.many)
            proof = E.decode_proof(nrp, st.rounds, st.final_lens, coms[0], p, lift.many)
            assert proof is not None                               # every mutation keeps the files well-formed
            want_ok.append(bool(mod.verify(st, proof, RP.sha256_oracle())))
            want_pts.append(st.backend.last)
        assert want_ok == [True] + [False] * len(ms)               # the only valid member is the honest one
        assert [e is None for e in want_pts] == want_ok
        coms_f, prfs = [c for _, c, _ in files], [p for _, _, p in files]
        try:
            for host_oracle_max in (0, len(files), 2**64 - 1):    # hashing on the device; on the host cores; the defaults
                nat.set_option("host_oracle_max", host_oracle_max)
                ok, status, _ = nat.verify_batch(coms_f, prfs, SEED, want_status=True)
                assert not ok and status == [VALID] + [INVALID] * len(ms), host_oracle_max
                each, pts = nat.verify_each(coms_f, prfs, want_points=True)
                assert each == status and pts == want_pts, host_oracle_max
                # the combined point: the weights restated from include/bppp.h over the CPU's points
                ok2, st2, chs, comb = _batch_full(gpu, nat, coms_f, prfs)
                assert (ok2, st2) == (ok, status)
                lead = nat.shape["challenges_per_proof"] - nat.shape["rounds"]
                rhos = [_rho(nat, SEED, b, chs[b][lead - 1], chs[b][lead] if nat.shape["rounds"] else 0, prfs[b]) for b in range(len(files))]
                assert comb == oracle_lib.inner_product([(r, e) for r, e in zip(rhos, want_pts) if e is not None]), host_oracle_max
                assert nat.verify_batch(coms_f[:1], prfs[:1], SEED) and nat.verify_each(coms_f[:1], prfs[:1], want_points=True) == ([VALID], [None])
        finally:
            nat.set_option("host_oracle_max", 2**64 - 1)
    finally:
        nat.close()


def _bump(pf, byte):
    d = bytearray(pf); d[byte] ^= 4
    return bytes(d)


def test_a_batch_of_1030_one_round_proofs(gpu, oracle_lib):
    """two proofs a tile in the verifier's shared-basis sums (csrc/nlbatch.hip vb_kt) at k = 1: the flag setup through the library's prover"""
    st, nat, _ = _native(gpu, oracle_lib, "flag", "NL")
    try:
        B = 1030
        inputs = [inputs_of("flag", [b % 2], b) for b in range(B)]
        files = nat.prove_batch(inputs, [b"few rounds large %04d" % b for b in range(B)])
        assert files[5] == E.encode_proof(4, host_prove(st, "flag", [1], 5, b"few rounds large 0005"))
        cf, pf = [c for c, _ in files], [p for _, p in files]
        ok, status, _ = nat.verify_batch(cf, pf, SEED, want_status=True)
        assert ok and status == [VALID] * B
        pf[3] = _bump(pf[3], 7); pf[700] = _bump(pf[700], 32 + 9); pf[1029] = _bump(pf[1029], 32 * 3 + 11)      # a norm scalar, two linear ones
        want = [INVALID if b in (3, 700, 1029) else VALID for b in range(B)]
        ok, status, _ = nat.verify_batch(cf, pf, SEED, want_status=True)
        assert not ok and status == want
        assert nat.verify_each(cf, pf) == want
    finally:
        nat.close()


def test_a_mixed_job_of_one_round_zero_rounds_and_the_64bit_example(gpu, oracle_lib):
    _, one, _ = _native(gpu, oracle_lib, "flag", "NL")
    _, zero, _ = _native(gpu, oracle_lib, "binary two bits", "NL")
    schema = json.load(open(os.path.join(EXAMPLES, "64bit", "schema.json")))
    ex = RP.NativeRangeProofs(gpu, RP.setup_from_schema(OracleBackend(oracle_lib), schema))
    try:
        assert (one.shape["rounds"], zero.shape["rounds"], ex.shape["rounds"]) == (1, 0, 3)
        f1 = one.prove_batch([inputs_of("flag", [b % 2], b) for b in range(5)], [b"mixed one %d" % b for b in range(5)])
        # verify_mixed takes no per-proof public amounts: the members of the k = 0 group all carry the setup's own (2)
        f0 = zero.prove_batch([inputs_of("binary two bits", [2], j) for j in range(4)], [b"mixed zero %d" % j for j in range(4)])
        wit = json.load(open(os.path.join(EXAMPLES, "64bit", "witness.json")))
        fx = ex.prove_batch([RP.inputs_from_witness(wit, b"mixed ex %d" % j) for j in range(3)], [b"mixed ex rand %d" % j for j in range(3)])
        split = lambda fs: ([c for c, _ in fs], [p for _, p in fs])
        groups = [(one,) + split(f1), (zero,) + split(f0), (ex,) + split(fx)]
        assert RP.verify_mixed(gpu, groups, SEED, want_status=True) == (True, [VALID] * 12)
        groups[0][2][2] = _bump(groups[0][2][2], 40)
        want = [VALID] * 12
        want[2] = INVALID
        assert RP.verify_mixed(gpu, groups, SEED, want_status=True) == (False, want)
        for h in (one, zero, ex):
            h.set_option("culprits", 1)
        assert RP.verify_mixed(gpu, groups, SEED, want_status=True) == (False, want)
    finally:
        one.close(); zero.close(); ex.close()
