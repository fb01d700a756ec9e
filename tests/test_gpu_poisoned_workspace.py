"""No entry point may rest on what an earlier call left in a grow-only workspace (csrc/ctx.hpp: "no entry point reads a workspace word that the same
call has not written").  Every measured call here runs directly after bppp_test_ctx_poison / bppp_test_rp_poison (include/bppp_test.h) have filled
every scratch buffer of the context, of every handle involved and of their twins, first with 0x00 and then with 0xA5, and is compared with the CPU
reference: the host protocol code over the CPU oracle, oracle/pyoracle.py for MSM points - never the library on another route.

Zero comes first, inside the same test function: a stale word wrongly used as a count or an index then stays inside its array and shows as a wrong
value, and the failed assertion ends the test before 0xA5, which covers what zero cannot (stale "valid" or "no fault" words, scalars >= n, points off
the curve).

Every measured call is preceded, on the same context and handle, by a warm call of the same kind, at least as large and on DIFFERENT inputs, so that
the buffers have capacity beyond the measured call's carve:  large A -> poison -> large A' -> poison -> small B;  and one sequence per family in which
the warm call is another entry point that shares ws / ws2.  No route is measured after another route on the same inputs."""
import ctypes as C
import functools
import hashlib
import json
import os
import random
import types

import numpy as np
import pytest

import msm_stages as S
import pyoracle as O
import test_gpu_prove_device as PD
from bulletproofspp_amd import capi
from bulletproofspp_amd import encoding as E
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import points_to_array, scalars_to_array
from test_few_rounds_host import SETUPS, PointBackend, inputs_of, make_setup, public_amount, with_public
from test_gpu_decode_conformance import Layout, Lift
from test_gpu_few_rounds import _mutants, _pool, batch_arrays, run_batch, weighted_sum
from test_gpu_msm_reduce_known_logs import _fmt
from test_gpu_msm_sort_stage import E as ENV
from test_gpu_msm_sort_stage import _scalars
from test_gpu_verify_each import SEED, _batch_full, _rho
from test_rangeproof import EXAMPLES

pytestmark = pytest.mark.gpu

N, P = O.N, O.P
BYTES = (0x00, 0xA5)
VALID, INVALID = 0, 1
ERR_ARG, ERR_POINT = -1, -4
MAX = 2**64 - 1


# ----------------------------------------------------------------------------- the harness
def poison(byte, ctxs, nats=()):
    """every scratch buffer of the contexts, of the handles and of their twins filled with `byte`: the bytes filled"""
    tlib, total, n = capi.load_test_library(), 0, C.c_uint64(0)
    for g in ctxs:
        assert tlib.bppp_test_ctx_poison(g.h, byte, C.byref(n)) == 0
        total += n.value
    for nat in nats:
        assert tlib.bppp_test_rp_poison(nat.h, byte, C.byref(n)) == 0
        total += n.value
    return total


def after_poison(call, want, warm, ctxs, nats=()):
    """for each byte, zero first: the warm call, poison, `call`, compared with the CPU reference `want`"""
    for byte in BYTES:
        warm()
        assert poison(byte, ctxs, nats) > 0
        got = call()
        assert got == want, "after poison 0x%02X" % byte


def sequence(steps, ctxs, nats=()):
    """steps = [(call, want)]: A -> poison -> A' -> poison -> B ...; every step but the first is measured, the step before it is its warm call"""
    for (warm, _), (call, want) in zip(steps, steps[1:]):
        after_poison(call, want, warm, ctxs, nats)


# ----------------------------------------------------------------------------- 1. MSM
NBASE = 256
MSM_BIG, MSM_SMALL = 20011, 301
# route: kind, window bits, the context's environment, (n, batch) of the two large calls and of the small one
MSM_ROUTES = {
    "device c13": ("msm", 13, (), (MSM_BIG, 1), (MSM_SMALL, 1)),
    "device c16 fq29": ("msm", 16, (), (MSM_BIG, 1), (MSM_SMALL, 1)),
    "device c16 sized": ("msm", 16, ENV(BPPP_ACC_SIZED=1, BPPP_ACC_FQ29=0), (MSM_BIG, 1), (MSM_SMALL, 1)),
    "batch shared c5": ("batch shared", 5, (), (303, 5), (MSM_SMALL, 3)),
    "batch per instance c8": ("batch own", 8, (), (303, 5), (MSM_SMALL, 3)),
    "registered basis c8": ("basis", 8, (), (MSM_SMALL, 3), (MSM_SMALL, 1)),
    "small": ("small", 0, (), (3001, 1), (MSM_SMALL, 1)),
    "host buffers": ("host", 0, (), (MSM_BIG, 1), (MSM_SMALL, 1)),
}


@pytest.fixture(scope="module")
def msm_contexts(gpu):
    made = S.make_contexts(gpu, [r[2] for r in MSM_ROUTES.values()])
    yield made
    S.close_contexts(made)


@functools.lru_cache(maxsize=None)
def _msm_base():
    pts = O.hash_points(b"poisoned workspace msm", 2 * NBASE)
    return pts, points_to_array(pts)


def _msm_rows(what, c, n, batch, flat, seed):
    rnd = random.Random("poisoned msm %s %d %d %d" % (what, c, n, seed))
    if what == "dense":
        return [[rnd.randrange(N) for _ in range(n)] for _ in range(batch)]
    if what == "few":                                               # few non-zero: nearly every bucket stays empty over the poison
        rows = [[0] * n for _ in range(batch)]
        for b in range(batch):
            for i in {0, 63 % n, 64 % n, n // 2, n - 1, rnd.randrange(n)}:
                rows[b][i] = rnd.randrange(1, N)
        return rows
    fmt = _fmt(c or 16, batch, flat)                                # the edge scalars of the sort-stage tests on this plan's digit format
    return [_scalars(fmt, n, 7000 + 10 * seed + b) for b in range(batch)]


def _msm_case(ec, kind, c, n, batch, what, seed):
    """(scalar rows, the index of every point in the base, the oracle's points): point i of instance b is base point (i + 7 b) mod 256, of the second
    half of the base for the odd instances of a per-instance batch.  The oracle adds the scalars of equal points first."""
    base, _ = _msm_base()
    rows = _msm_rows(what, c, n, batch, kind == "basis", seed)
    own = kind == "batch own"
    idx = [[(i + (7 * b if own else 0)) % NBASE + (NBASE if own and b % 2 else 0) for i in range(n)] for b in range(batch)]
    want = []
    for b in range(batch):
        acc = {}
        for s, j in zip(rows[b], idx[b]):
            acc[j] = (acc.get(j, 0) + s) % N
        terms = [(s, base[j]) for j, s in acc.items() if s]
        want.append(ec.inner_product(terms) if terms else None)
    return rows, idx, want


def _msm_call(g, kind, c, n, batch, rows, idx, basis=None):
    _, base_arr = _msm_base()
    sc = scalars_to_array([s for r in rows for s in r])
    if kind == "host":
        return lambda: [g.msm(sc, np.ascontiguousarray(base_arr[idx[0]]))]
    pts = np.ascontiguousarray(base_arr[[j for r in (idx if kind == "batch own" else idx[:1]) for j in r]])

    def call():
        ds, dp = g.to_device(sc), g.to_device(pts)
        try:
            if kind in ("msm", "small"):
                return [g.msm_device(ds, dp, n, window_bits=c)]
            if kind == "basis":
                return basis.msm(ds, n, batch)
            return g.msm_batch_device(ds, dp, n, batch, shared_points=kind == "batch shared", window_bits=c)
        finally:
            g.free(ds); g.free(dp)
    return call


def _reduce_route(g):
    rep = capi.TestReduceReport()
    assert capi.load_test_library().bppp_test_last_reduce(g.h, C.byref(rep)) == 0
    return rep.route


@pytest.mark.parametrize("route", list(MSM_ROUTES))
def test_msm_after_poison(msm_contexts, oracle_lib, route):
    kind, c, env, (n_big, b_big), (n_small, b_small) = MSM_ROUTES[route]
    g = msm_contexts[env]
    basis = None
    if kind == "basis":                                             # the table is persistent: built once, never poisoned
        basis = g.basis(np.ascontiguousarray(_msm_base()[1][np.arange(n_big) % NBASE]), window_bits=c, batch_hint=b_big)
    try:
        steps = []
        for what, n, batch, seed in (("dense", n_big, b_big, 1), ("few", n_big, b_big, 2), ("dense", n_big, b_big, 3), ("edge", n_small, b_small, 4), ("few", n_small, b_small, 5)):
            rows, idx, want = _msm_case(oracle_lib, kind, c, n, batch, what, seed)
            steps.append((_msm_call(g, kind, c, n, batch, rows, idx, basis), want))
        sequence(steps, [g])
        if kind == "msm":
            assert S.hooks(g)[2:] == {"device c13": (0, 0), "device c16 fq29": (1, 1), "device c16 sized": (1, 0)}[route]
        if kind == "small":
            assert _reduce_route(g) == 0                            # k_msm_small: the route the name claims
    finally:
        if basis is not None:
            basis.close()


# ----------------------------------------------------------------------------- 2. the argument verifiers
ARG_SHAPES = {("NL", 7, 2): 1, ("NL", 9, 5): 2, ("IP", 7, 2): 1, ("IP", 5, 3): 2}


@pytest.mark.parametrize("kind,c", [("msm", 13), ("msm", 16), ("small", 0), ("host", 0)])
def test_msm_after_an_argument_batch(gpu, oracle_lib, kind, c):
    """cross-kind: the warm call is an argument batch of 70, whose assembly lies in ws2 and whose MSM (another plan) in ws; then an MSM of 301 terms"""
    pool = _pool(oracle_lib, ("NL", 9, 5), 2)
    arrs, _ = _arg_batch(oracle_lib, pool, 70, 7)

    def warm():
        assert run_batch(gpu, pool, 70, arrs)[0] == 0
    for what, seed in (("few", 11), ("edge", 12)):
        rows, idx, want = _msm_case(oracle_lib, kind, c, MSM_SMALL, 1, what, seed)
        after_poison(_msm_call(gpu, kind, c, MSM_SMALL, 1, rows, idx), want, warm, [gpu])


def _arg_batch(ec, pool, B, salt):
    """a batch of B with every third member changed in one place (another place and another proof for every salt), its weights, the oracle's sum"""
    rnd = random.Random("poisoned args %s %d %d %d %d" % (pool.flavour, pool.nl, pool.ll, B, salt))
    nplaces = len(pool.changed[0])
    members = [pool.changed[(b + salt) % 3][(b + 5 * salt) % nplaces][1] if (b + salt) % 3 == 0 else pool.honest[(b + salt) % 3] for b in range(B)]
    rhos = [rnd.randrange(1, N) for _ in range(B)]
    want = weighted_sum(ec, rhos, [pool.point(v) for v in members])
    assert want is not None
    return batch_arrays(pool, members, rhos), want


@pytest.mark.parametrize("flavour,nl,ll", list(ARG_SHAPES))
def test_argument_verifier_after_poison(gpu, oracle_lib, flavour, nl, ll):
    key = (flavour, nl, ll)
    pool = _pool(oracle_lib, key, ARG_SHAPES[key])
    steps = []
    for B, salt in ((33, 1), (33, 2), (5, 3)):
        arrs, want = _arg_batch(oracle_lib, pool, B, salt)
        steps.append((functools.partial(run_batch, gpu, pool, B, arrs), (0, want)))
    rnd = random.Random("poisoned args honest %r" % (key,))
    rhos = [rnd.randrange(1, N) for _ in range(5)]
    honest = batch_arrays(pool, [pool.honest[b % 3] for b in range(5)], rhos)
    steps.append((functools.partial(run_batch, gpu, pool, 5, honest), (0, None)))      # an honest batch: accepted by its own point, after a rejected one
    sequence(steps, [gpu])
    # a refusal as the warm call: the flag word it raised, and the poison over it, must not refuse (or accept) the batch that follows
    zero_rho = {k: a.copy() for k, a in honest.items()}
    zero_rho["rho"][1] = 0
    off_curve = {k: a.copy() for k, a in honest.items()}
    x, y = capi.array_to_point(off_curve["resp"][0])
    off_curve["resp"][0] = points_to_array([(x, (y + 1) % P)])[0]
    mixed, want = _arg_batch(oracle_lib, pool, 5, 4)
    for bad, code in ((zero_rho, ERR_ARG), (off_curve, ERR_POINT)):
        def refused():
            assert run_batch(gpu, pool, 5, bad)[0] == code
        refused()
        assert run_batch(gpu, pool, 5, honest) == (0, None)         # directly after it, nothing poisoned: the stale flag word
        after_poison(functools.partial(run_batch, gpu, pool, 5, honest), (0, None), refused, [gpu])
        after_poison(functools.partial(run_batch, gpu, pool, 5, mixed), (0, want), refused, [gpu])


def test_argument_verifier_after_an_msm_and_a_prover(gpu, oracle_lib):
    """cross-kind: the warm call is an MSM over ws, then a range-proof prove batch, both larger than the verified batch"""
    key = ("NL", 9, 5)
    pool = _pool(oracle_lib, key, ARG_SHAPES[key])
    arrs, want = _arg_batch(oracle_lib, pool, 5, 6)
    rows, idx, _ = _msm_case(oracle_lib, "msm", 13, MSM_BIG, 1, "dense", 9)
    after_poison(functools.partial(run_batch, gpu, pool, 5, arrs), (0, want), _msm_call(gpu, "msm", 13, MSM_BIG, 1, rows, idx), [gpu])


# ----------------------------------------------------------------------------- range proofs: setups, host proofs, references
RP_KEYS = [("flag", "NL"), ("binary two bits", "NL"), ("shared flag", "IP"), ("32bit", None)]
_HOST = {}


def _example(name):
    return json.load(open(os.path.join(EXAMPLES, name, "schema.json"))), json.load(open(os.path.join(EXAMPLES, name, "witness.json")))


def _host_setup(ec, key):
    """(setup over the CPU oracle whose verifier keeps the committed point, binary)"""
    if key not in _HOST:
        name, flavour = key
        if name in SETUPS:
            _HOST[key] = (make_setup(PointBackend(ec), name, flavour), SETUPS[name][0])
        else:
            schema = _example(name)[0]
            binary = bool(schema.get("binary", False))
            _HOST[key] = ((BRP if binary else RP).setup_from_schema(PointBackend(ec), schema), binary)
    return _HOST[key]


def _native(gpu, ec, key, **options):
    st, binary = _host_setup(ec, key)
    nat = (BRP.NativeBinaryRangeProofs if binary else RP.NativeRangeProofs)(gpu, st)
    for k, v in options.items():
        nat.set_option(k, v)
    return nat


def _amounts(key, j, vary):
    """the amounts of proof j of a small setup: the table's three witnesses in turn when `vary`, else the first (a conserved setup then needs no
    per-proof public amount)"""
    return SETUPS[key[0]][4][j % 3 if vary else 0]


def _rows(ec, key, j, vary=False):
    """the prover's rows of proof j: other blindings for every j, other amounts where the setup allows"""
    name = key[0]
    if name in SETUPS:
        return inputs_of(name, _amounts(key, j, vary), "poisoned %d" % j)
    _, binary = _host_setup(ec, key)
    rows = RP.inputs_from_witness(_example(name)[1], b"poisoned %s %d" % (name.encode(), j))
    return [(v, bl) for v, _, bl in rows] if binary else rows


def _prefix(j):
    return b"poisoned workspace rnd %04d" % j


@functools.lru_cache(maxsize=None)
def _proof_cached(key, j, vary, binding):
    ec = O.CEC()
    st, binary = _host_setup(ec, key)
    mod = BRP if binary else RP
    if key[0] in SETUPS:
        st = with_public(st, key[0], _amounts(key, j, vary))
    proof = mod.prove(st, mod.witness(st, _rows(ec, key, j, vary)), RP.sha256_oracle(binding), RP.hash_to_scalar(_prefix(j)))
    return E.encode_proof(2 if binary else 4, proof)


def host_files(key, js, vary=False, bindings=None):
    """[(commitments file, proof file)] of the host protocol's proofs js"""
    return [_proof_cached(key, j, vary, b"" if bindings is None else bindings[i]) for i, j in enumerate(js)]


def _publics(key, js, vary):
    """prove_batch's per-proof public amounts for proofs js, None for a setup without one"""
    name = key[0]
    if name not in SETUPS or public_amount(name, _amounts(key, js[0], vary)) is None:
        return None
    amts = [public_amount(name, _amounts(key, j, vary)) for j in js]
    return amts if SETUPS[name][0] else [[a] for a in amts]


def _shape(st, binary, cf, pf):
    return {"nranges": len(st.rds), "rounds": st.rounds, "final_norm": st.final_lens[0], "final_lin": st.final_lens[1], "coms_bytes": len(cf), "proof_bytes": len(pf),
            "challenges_per_proof": (4 if binary else 7) + st.rounds}


@functools.lru_cache(maxsize=None)
def _verifier_case(key, j, limit):
    """the honest files of host proof j and its single-field mutants (all of them, or the first `limit` files), with the host protocol verifier's verdict,
    the point it commits, and verify_batch's weight of every file at its position in the batch: (files, statuses, points, rhos)"""
    ec = O.CEC()
    st, binary = _host_setup(ec, key)
    mod, nrp = (BRP if binary else RP), (2 if binary else 4)
    cf, pf = host_files(key, [j])[0]
    shape = _shape(st, binary, cf, pf)
    L, lift = Layout(shape, nrp), Lift(ec)
    files = ([(cf, pf)] + [(c, p) for _, c, p in _mutants(L, cf, pf)])[:limit]
    status, pts, rhos = [], [], []
    holder = types.SimpleNamespace(shape=shape)                     # what _rho reads of a handle
    for b, (c, p) in enumerate(files):
        coms = E.decode_commitments(L.nr, c, lift.many)
        proof = E.decode_proof(nrp, st.rounds, st.final_lens, coms[0], p, lift.many)
        assert proof is not None
        ok = bool(mod.verify(st, proof, RP.sha256_oracle()))
        assert ok == (st.backend.last is None)
        status.append(VALID if ok else INVALID)
        pts.append(st.backend.last)
        lead, es = mod.verifier_challenges(st, proof, RP.sha256_oracle())
        rhos.append(_rho(holder, SEED, b, lead[-1], es[0] if st.rounds else 0, p))
    assert status == [VALID] + [INVALID] * (len(files) - 1)
    terms = [(r, e) for r, e in zip(rhos, pts) if e is not None]
    return files, status, pts, (ec.inner_product(terms) if terms else None)


# ----------------------------------------------------------------------------- 3. the range-proof verifier
VERIFY_ROUTES = {"device oracle": dict(host_oracle_max=0), "host oracle": dict(host_oracle_max=MAX), "culprits, one pass": dict(host_oracle_max=0, culprits=1)}


def _verify_calls(gpu, nat, case):
    files, status, pts, comb = case
    cf, pf = [c for c, _ in files], [p for _, p in files]
    ok = all(s == VALID for s in status)
    return [(lambda: tuple(nat.verify_batch(cf, pf, SEED, want_status=True)[:2]), (ok, status)),
            (lambda: tuple(nat.verify_each(cf, pf, want_points=True)), (status, pts)),
            (lambda: (lambda r: (r[0], r[1], r[3]))(_batch_full(gpu, nat, cf, pf)), (ok, status, comb))]


@pytest.mark.parametrize("route", list(VERIFY_ROUTES))
def test_rp_verifier_after_poison(gpu, oracle_lib, route):
    for key in RP_KEYS:
        nat = _native(gpu, oracle_lib, key, **VERIFY_ROUTES[route])
        try:
            cases = [_verifier_case(key, 0, None), _verifier_case(key, 1, None), _verifier_case(key, 2, 5), _verifier_case(key, 3, 1)]     # A, A', B, one honest file
            per_entry = zip(*[_verify_calls(gpu, nat, case) for case in cases])
            for steps in per_entry:                                 # verify_batch with status; verify_each with points; the combined point
                sequence(list(steps), [gpu], [nat])
        finally:
            nat.close()


def test_rp_verify_mixed_after_poison(gpu, oracle_lib):
    keys = [("flag", "NL"), ("binary two bits", "NL")]
    nats = [_native(gpu, oracle_lib, key, host_oracle_max=0) for key in keys]
    try:
        def job(js, limit):
            groups, want = [], []
            for nat, key, j in zip(nats, keys, js):
                files, status, _, _ = _verifier_case(key, j, limit)
                groups.append((nat, [c for c, _ in files], [p for _, p in files]))
                want += status
            return (lambda: tuple(RP.verify_mixed(gpu, groups, SEED, want_status=True))), (all(s == VALID for s in want), want)
        sequence([job((0, 1), None), job((1, 2), None), job((2, 3), 3), job((3, 0), 1)], [gpu], nats)
    finally:
        for nat in nats:
            nat.close()


def test_rp_verifier_after_a_prover_and_an_argument_batch(gpu, oracle_lib):
    """cross-kind: an argument batch of 70 and a prove batch on the same handle come first; then a verification of 5 files"""
    key = ("32bit", None)
    nat = _native(gpu, oracle_lib, key, host_oracle_max=0)
    pool = _pool(oracle_lib, ("NL", 9, 5), 2)
    arrs, _ = _arg_batch(oracle_lib, pool, 70, 8)
    try:
        def warm():
            assert run_batch(gpu, pool, 70, arrs)[0] == 0
            nat.prove_batch([_rows(oracle_lib, key, j) for j in (10, 11, 12)], [_prefix(j) for j in (10, 11, 12)])
        for call, want in _verify_calls(gpu, nat, _verifier_case(key, 2, 5)):
            after_poison(call, want, warm, [gpu], [nat])
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 4. the provers
COMB = dict(comb_min=1, comb_bits=7)
# route: the handle's options; `table`: one proof first so that the comb table (persistent) exists before the option that would keep it from being built
PROVE_ROUTES = {
    "default": dict(),
    "comb stream, device oracle": dict(COMB, host_oracle_max=0),
    "comb stream, host oracle": dict(COMB, host_oracle_max=MAX),
    "host algebra": dict(COMB, table=True, host_algebra=1),
    "fold points": dict(COMB, table=True, fold_points=1),
    "split, twin handle": dict(COMB, host_oracle_max=0, split_min=2),
    "rebased": dict(COMB, host_oracle_max=0),
    "device entry point": dict(COMB, host_oracle_max=0),
    "status device entry point, one refused": dict(COMB, host_oracle_max=0),
    "per-proof public amounts": dict(COMB, host_oracle_max=0),
    "bound": dict(COMB, host_oracle_max=0),
}
PROVE_KEYS = {"rebased": [("bin_test", None)], "per-proof public amounts": [("flag typed", "NL"), ("binary two bits", "NL")],
              "status device entry point, one refused": [("flag", "NL"), ("shared flag", "IP"), ("32bit", None)]}
A, A2, B = (20, 21, 22), (23, 24, 25), (26,)                       # the proofs of the two large batches and of the small one


def _prove_step(gpu, ec, nat, key, route, js):
    vary = route == "per-proof public amounts"
    inputs, prefixes = [_rows(ec, key, j, vary) for j in js], [_prefix(j) for j in js]
    if route == "bound":
        bindings = [hashlib.sha256(b"poisoned binding %d" % j).digest() for j in js]
        return (lambda: nat.prove_batch(inputs, prefixes, bindings=bindings)), host_files(key, js, bindings=tuple(bindings))
    if route == "device entry point":
        return (lambda: PD._device_files(nat, inputs, prefixes)), host_files(key, js)
    if route == "status device entry point, one refused":
        bad = len(js) // 2                                          # that proof's first amount lies above its range: refused, the others proved
        rows = [list(r) for r in inputs]
        rows[bad][0] = (_host_setup(ec, key)[0].rds[0].hi + 3,) + tuple(rows[bad][0][1:])
        zero = (bytes(nat.shape["coms_bytes"]), bytes(nat.shape["proof_bytes"]))
        want = [zero if i == bad else f for i, f in enumerate(host_files(key, js))]
        status = [capi.RP_WIT_OUT_OF_RANGE if i == bad else capi.RP_WIT_OK for i in range(len(js))]

        def call():
            with PD._DeviceCall(nat, rows, prefixes) as dc:
                d = dc.d
                gpu.upload(d["cf"], np.full(dc.cf.nbytes, 0xEE, dtype=np.uint8))
                gpu.upload(d["pf"], np.full(dc.pf.nbytes, 0xEE, dtype=np.uint8))
                st = nat.prove_batch_status_device(dc.B, d["amt"], 0 if dc.binary else d["typ"], d["bld"], d["pre"], dc.plen, d["cf"], d["pf"])
                return [int(s) for s in st], nat._prove_files(dc.B, gpu.download(d["cf"], dc.cf.shape, np.uint8), gpu.download(d["pf"], dc.pf.shape, np.uint8))
        return call, (status, want)
    pubs = _publics(key, js, vary)
    return (lambda: nat.prove_batch(inputs, prefixes, public_amounts=pubs)), host_files(key, js, vary)


@pytest.mark.parametrize("route", list(PROVE_ROUTES))
def test_prover_after_poison(gpu, oracle_lib, monkeypatch, route):
    if route == "rebased":
        monkeypatch.setenv("BPPP_NLB_REBASE", "2")                  # read when the argument starts
    if route == "split, twin handle":
        monkeypatch.setenv("BPPP_RP_SPLIT_MIN_BINARY", "2")         # a binary handle takes its split threshold when it is created
    options = dict(PROVE_ROUTES[route])
    table = options.pop("table", False)
    late = {k: options.pop(k) for k in ("host_algebra", "fold_points") if k in options}
    for key in PROVE_KEYS.get(route, RP_KEYS):
        nat = _native(gpu, oracle_lib, key, **options)
        try:
            if table:
                nat.prove_batch([_rows(oracle_lib, key, 19)], [_prefix(19)])
            for k, v in late.items():
                nat.set_option(k, v)
            sequence([_prove_step(gpu, oracle_lib, nat, key, route, js) for js in (A, A2, B)], [gpu], [nat])
        finally:
            nat.close()


def test_prover_after_a_verifier(gpu, oracle_lib):
    """cross-kind: a verification of 70 files on the same handle and context, then a prove batch of 3"""
    for key in (("flag", "NL"), ("32bit", None)):
        nat = _native(gpu, oracle_lib, key, host_oracle_max=0, **COMB)
        try:
            files = (_verifier_case(key, 0, None)[0] * 70)[:70]
            cf, pf = [c for c, _ in files], [p for _, p in files]

            def warm():
                assert not nat.verify_batch(cf, pf, SEED)
            call, want = _prove_step(gpu, oracle_lib, nat, key, "default", A)
            after_poison(call, want, warm, [gpu], [nat])
        finally:
            nat.close()


# ----------------------------------------------------------------------------- 5. the balance calls
BAL_NAMES = ["rec_test", "bin_test"]                                # one typed and one binary setup of test_gpu_commit_open
BAL_SEED = hashlib.sha256(b"poisoned balance seed").digest()
AUX = hashlib.sha256(b"poisoned balance aux").digest()
OK, MISMATCH, MALFORMED = 0, 1, 2
MASK = RP.TALLY_SUBTRACT - 1


def _chunks(nat, flat, tally=8):
    """the items of one pass lowered, so that the jobs below take several passes over the poisoned workspace"""
    tlib = capi.load_test_library()
    assert tlib.bppp_test_rp_set_flat_chunk(nat.h, flat) == 0 and tlib.bppp_test_rp_set_tally_chunk(nat.h, tally) == 0


class Balance:
    """One job over `rows` of test_gpu_commit_open's pool of a setup: sums of a few signed entries, their claims, keys and signatures - all by the host
    protocol code over the CPU oracle - with one mismatch and one malformed member in every verifying call.  calls = {name: (handle -> call, want)}."""

    def __init__(self, ec, name, rows, salt, nsums):
        from rp_backends import OracleBackend
        import test_gpu_commit_open as CO
        from test_gpu_excess_keys import _s_of, _with_s
        st, inputs, triples, pts, files = CO._case(ec, name)
        be, binary, nr = OracleBackend(ec), name == "bin_test", len(st.rds)
        rng = random.Random("poisoned balance %s %d" % (name, salt))
        g, H0, Bp = RP._excess_bases(st)
        inputs, files, triples = [inputs[r] for r in rows], [files[r] for r in rows], [triples[r] for r in rows]
        flat_t, flat_p = [t for row in triples for t in row], [p for r in rows for p in pts[r]]
        total = len(flat_t)
        ss, en = [0], []
        for t in range(nsums):
            en += [RP.tally_entry(rng.randrange(total), rng.random() < 0.5) for _ in range(2 + (t + salt) % 4)]
            ss.append(len(en))
        claims = RP.tally_claims_host(flat_t, ss, en)
        S = RP.tally_sums(be, flat_p, ss, en)
        cut = (lambda c: (c[0], c[2])) if binary else (lambda c: tuple(c))       # a claim as the wrappers of this handle take it
        # the malformed member: the first commitment that sum 2 gathers has an x without a curve point; the mismatch: the first sum that does not gather it
        m = en[ss[2]] & MASK
        malf = [any(e & MASK == m for e in en[ss[t]:ss[t + 1]]) for t in range(nsums)]
        mis = malf.index(False)
        files_bad = list(files)
        files_bad[m // nr] = CO._set_x(files[m // nr], nr, m % nr, CO._no_point_x(ec))
        claims_mis = list(claims)
        claims_mis[mis] = ((claims[mis][0] + 1) % N,) + tuple(claims[mis][1:])
        want_sums = [MALFORMED if malf[t] else MISMATCH if t == mis else OK for t in range(nsums)]
        want_mis = [MISMATCH if t == mis else OK for t in range(nsums)]
        c = {}
        # ---- commit and open
        c["commit"] = lambda nat: (lambda: nat.commit_batch(inputs)), files
        o = (m + 1) % total                                         # the opening claimed with another amount
        inputs_mis = [list(r) for r in inputs]
        inputs_mis[o // nr][o % nr] = (inputs[o // nr][o % nr][0] + 1,) + tuple(inputs[o // nr][o % nr][1:])
        triples_mis = [list(r) for r in triples]
        triples_mis[o // nr][o % nr] = (triples[o // nr][o % nr][0] + 1,) + tuple(triples[o // nr][o % nr][1:])
        grid = lambda cells: [[cells.get(b * nr + i, OK) for i in range(nr)] for b in range(len(rows))]
        c["open each"] = lambda nat: (lambda: nat.open_each(files_bad, inputs_mis)), grid({o: MISMATCH, m: MALFORMED})
        rho = CO._job_weight(None, st, BAL_SEED, 0, files, triples_mis, o // nr, o % nr)
        c["open batch, point"] = lambda nat: (lambda: nat.open_batch(files, inputs_mis, BAL_SEED, want_status=True, want_point=True)), (False, grid({o: MISMATCH}), ec.mul((-rho) % N, g))
        c["open batch, statuses"] = lambda nat: (lambda: nat.open_batch(files_bad, inputs_mis, BAL_SEED, want_status=True)), (False, grid({o: MISMATCH, m: MALFORMED}), None)
        c["open batch, honest"] = lambda nat: (lambda: nat.open_batch(files, inputs, BAL_SEED, want_status=True, want_point=True)), (True, grid({}), None)
        # ---- tallies
        wcl, wmis = [cut(x) for x in claims], [cut(x) for x in claims_mis]
        c["tally each"] = lambda nat: (lambda: nat.tally_each(files_bad, ss, en, wmis, want_points=True)), (want_sums, [None if malf[t] else S[t] for t in range(nsums)])
        a1, ty1, e1 = claims_mis[mis]
        rho = RP.tally_weight(BAL_SEED, mis, a1, 0 if binary else ty1, e1)
        c["tally batch, point"] = lambda nat: (lambda: nat.tally_batch(files, ss, en, wmis, BAL_SEED, want_status=True, want_point=True)), (False, want_mis, ec.mul((-rho) % N, g))
        c["tally batch, statuses"] = lambda nat: (lambda: nat.tally_batch(files_bad, ss, en, wmis, BAL_SEED, want_status=True)), (False, want_sums, None)
        c["tally batch, honest"] = lambda nat: (lambda: nat.tally_batch(files, ss, en, wcl, BAL_SEED, want_status=True, want_point=True)), (True, [OK] * nsums, None)
        c["tally claims"] = lambda nat: (lambda: nat.tally_claims(inputs, ss, en)), wcl
        # ---- excess signatures over the sums
        es = [x[2] for x in claims]
        msgs = [hashlib.sha256(b"poisoned msg %d %d" % (salt, t)).digest() for t in range(nsums)]
        signed = [RP.excess_sign_host(be, st, e, mg, AUX) for e, mg in zip(es, msgs)]
        assert all(s[0] == 0 for s in signed)
        sigs, Xs = [s[1] for s in signed], [s[2] for s in signed]
        c["excess sign"] = lambda nat: (lambda: nat.excess_sign(es, msgs, AUX, want_status=True, want_points=True)), (sigs, [OK] * nsums, Xs)
        sigs_bad = list(sigs)
        sigs_bad[mis] = _with_s(sigs[mis], (_s_of(sigs[mis]) + 1) % N)
        pub = [x[:1] if binary else x[:2] for x in claims]
        want = [RP.excess_verify_host(be, st, S[t], claims[t] if not binary else (claims[t][0],), msgs[t], sigs_bad[t], malformed=malf[t]) for t in range(nsums)]
        assert want == want_sums
        c["excess verify each"] = lambda nat: (lambda: nat.excess_verify_each(files_bad, ss, en, pub, msgs, sigs_bad)), want
        c["excess verify batch"] = lambda nat: (lambda: nat.excess_verify_batch(files_bad, ss, en, pub, msgs, sigs_bad, BAL_SEED, want_status=True)), (False, want, None)
        c["excess verify batch, honest"] = lambda nat: (lambda: nat.excess_verify_batch(files, ss, en, pub, msgs, sigs, BAL_SEED, want_status=True, want_point=True)), (True, [OK] * nsums, None)
        # ---- stated keys
        keys = [RP.excess_key33(X) for X in Xs]
        c["excess keys"] = lambda nat: (lambda: nat.excess_keys(es, want_status=True)), (keys, [OK] * nsums)
        keys_bad = list(keys)
        keys_bad[2] = keys[2][:32] + b"\x02"                        # a sign byte above 1: no key
        want_k = [RP.excess_verify_key_host(be, st, keys_bad[t], msgs[t], sigs_bad[t]) for t in range(nsums)]
        assert want_k[2] == RP.EXCESS_BAD_KEY and want_k[mis] == MISMATCH and sum(want_k) == RP.EXCESS_BAD_KEY + MISMATCH
        c["excess verify keys each"] = lambda nat: (lambda: nat.excess_verify_keys_each(keys_bad, msgs, sigs_bad)), want_k
        c["excess verify keys batch"] = lambda nat: (lambda: nat.excess_verify_keys_batch(keys_bad, msgs, sigs_bad, BAL_SEED, want_status=True)), (False, want_k, None)
        c["excess verify keys batch, honest"] = lambda nat: (lambda: nat.excess_verify_keys_batch(keys, msgs, sigs, BAL_SEED, want_status=True, want_point=True)), (True, [OK] * nsums, None)
        # sums against stated keys: sum t has t mod 3 keys of its own, the offset takes the rest of the blinding sum
        ks, xs, off = [0], [], []
        for t in range(nsums):
            mine = [rng.randrange(1, N) for _ in range(t % 3)]
            xs += mine
            ks.append(len(xs))
            off.append((es[t] - sum(mine)) % N)
        skeys = [RP.excess_key33(be.commit([x], [Bp])) for x in xs]
        cl3 = [(claims_mis[t][0], claims_mis[t][1], off[t]) for t in range(nsums)]
        hosted = [RP.excess_sums_host(be, st, S[t], cl3[t] if not binary else (cl3[t][0], cl3[t][2]), skeys[ks[t]:ks[t + 1]], malformed=malf[t]) for t in range(nsums)]
        assert [h[0] for h in hosted] == want_sums
        w3 = [cut(x) for x in cl3]
        c["excess sums each"] = lambda nat: (lambda: nat.excess_sums_each(files_bad, ss, en, w3, ks, skeys, want_points=True)), ([h[0] for h in hosted], [h[1] for h in hosted])
        c["excess sums batch"] = lambda nat: (lambda: nat.excess_sums_batch(files_bad, ss, en, w3, ks, skeys, BAL_SEED, want_status=True)), (False, want_sums, None)
        # ---- the multi-party signer: every sum's blinding in two parts
        ps, pe, pm = [0], [], []
        for t in range(nsums):
            first = rng.randrange(1, N)
            pe += [first, (es[t] - first) % N]
            pm += [msgs[t]] * 2
            ps.append(len(pe))
        nonces = [RP.excess_part_nonces_host(be, st, e, mg, AUX) for e, mg in zip(pe, pm)]
        assert all(s == 0 for s, _ in nonces)
        pn = [b for _, b in nonces]
        pk = [RP.excess_key33(be.commit([e], [Bp])) for e in pe]
        c["part nonces"] = lambda nat: (lambda: nat.excess_part_nonces(pe, pm, AUX, want_status=True)), (pn, [OK] * len(pe))
        agg = [RP.excess_part_aggregate_host(be, st, pn[ps[t]:ps[t + 1]], pk[ps[t]:ps[t + 1]]) for t in range(nsums)]
        assert all(a[0] == 0 for a in agg)
        an, ak = [a[1] for a in agg], [a[2] for a in agg]
        c["part aggregate"] = lambda nat: (lambda: nat.excess_part_aggregate(ps, pn, pk, want_status=True)), (an, ak, [OK] * nsums)
        an2, ak2 = [an[i // 2] for i in range(len(pe))], [ak[i // 2] for i in range(len(pe))]
        parts = [RP.excess_part_sign_host(be, st, pe[i], pm[i], AUX, an2[i], ak2[i]) for i in range(len(pe))]
        assert all(s == 0 for s, _ in parts)
        partials = [b for _, b in parts]
        c["part sign"] = lambda nat: (lambda: nat.excess_part_sign(pe, pm, AUX, an2, ak2, want_status=True)), (partials, [OK] * len(pe))
        partials_bad = list(partials)
        partials_bad[3] = RP._put((RP._get256(partials[3]) + 1) % N)
        ver = [RP.excess_part_verify_host(be, st, pn[ps[t]:ps[t + 1]], pk[ps[t]:ps[t + 1]], partials_bad[ps[t]:ps[t + 1]], msgs[t]) for t in range(nsums)]
        want_parts = [v for per, _ in ver for v in per]
        assert want_parts == [MISMATCH if i == 3 else OK for i in range(len(pe))]
        c["part verify"] = lambda nat: (lambda: nat.excess_part_verify(ps, pn, pk, partials_bad, msgs)), (want_parts, [s for _, s in ver])
        comb = [RP.excess_part_combine_host(be, st, pn[ps[t]:ps[t + 1]], pk[ps[t]:ps[t + 1]], partials[ps[t]:ps[t + 1]], msgs[t]) for t in range(nsums)]
        c["part combine"] = lambda nat: (lambda: nat.excess_part_combine(ps, pn, pk, partials, msgs, want_status=True, want_keys=True)), ([x[1] for x in comb], [x[0] for x in comb], [x[2] for x in comb])
        self.calls, self.parts = c, {"part nonces", "part aggregate", "part sign", "part verify", "part combine"}
        # the job's honest values, for callers that build calls of their own (tests/test_gpu_guarded_outputs.py)
        self.v = types.SimpleNamespace(inputs=inputs, files=files, sum_start=ss, entries=en, claims=wcl, blinds=es, msgs=msgs, sigs=sigs, excess_points=Xs, keys=keys,
                                       part_start=ps, part_blinds=pe, part_msgs=pm, part_nonces=pn, part_keys=pk, agg_nonces=an, agg_keys=ak, partials=partials,
                                       combined=comb)


_BALANCE = {}
BAL_CALLS = ["commit", "open each", "open batch, point", "open batch, statuses", "open batch, honest", "tally each", "tally batch, point", "tally batch, statuses",
             "tally batch, honest", "tally claims", "excess sign", "excess verify each", "excess verify batch", "excess verify batch, honest", "excess keys",
             "excess verify keys each", "excess verify keys batch", "excess verify keys batch, honest", "excess sums each", "excess sums batch", "part nonces",
             "part aggregate", "part sign", "part verify", "part combine"]


def _balance(ec, name):
    """the jobs A, A', B of a setup: 24, 24 and 5 rows, 7, 7 and 4 sums, no row and no sum in common"""
    if name not in _BALANCE:
        _BALANCE[name] = [Balance(ec, name, list(range(0, 24)), 1, 7), Balance(ec, name, list(range(24, 48)), 2, 7), Balance(ec, name, list(range(60, 65)), 3, 4)]
    return _BALANCE[name]


@pytest.fixture(scope="module")
def balance_handles(gpu, oracle_lib):
    import test_gpu_commit_open as CO
    made = {name: CO._native(gpu, CO._case(oracle_lib, name)[0]) for name in BAL_NAMES}
    yield made
    for nat in made.values():
        nat.close()


@pytest.mark.parametrize("what", BAL_CALLS)
def test_balance_call_after_poison(gpu, oracle_lib, balance_handles, what):
    for name in BAL_NAMES:
        nat, jobs = balance_handles[name], _balance(oracle_lib, name)
        assert set(jobs[0].calls) == set(BAL_CALLS)
        _chunks(nat, 8 if what in jobs[0].parts else 4)             # a group of two parts is not split over passes: two parts a pass there
        steps = []
        for job in jobs:
            make, want = job.calls[what]
            steps.append(((lambda f: lambda: _plain(f()))(make(nat)), _plain(want)))
        sequence(steps, [gpu], [nat])


def _plain(v):
    """tuples as lists, recursively: the wrappers return either"""
    return [_plain(x) for x in v] if isinstance(v, (tuple, list)) else v


def test_balance_call_after_another_kind(gpu, oracle_lib, balance_handles):
    """cross-kind on one handle: a tally of 24 rows, then an excess signature of 4 sums; a key check, then a commit of 5 rows"""
    for name in BAL_NAMES:
        nat, (big, _, small) = balance_handles[name], _balance(oracle_lib, name)
        _chunks(nat, 4)
        for warm, measured in (("tally batch, statuses", "excess sign"), ("excess verify keys batch", "commit"), ("commit", "tally each"), ("open batch, point", "excess sums each")):
            make, want = small.calls[measured]
            after_poison((lambda f: lambda: _plain(f()))(make(nat)), _plain(want), big.calls[warm][0](nat), [gpu], [nat])


# ---- the block call
def _block_job(ec, name, js, rows, salt, wrong):
    """a block over host proofs js (the first rows of the pool) and rows `rows` of test_gpu_commit_open's pool: (arguments of verify_block, want).
    wrong: proof 1 tampered in a final scalar, signature 0 with s + 1, the amount of sum 0 off by one, and sum 2 gathers an x without a curve point."""
    from rp_backends import OracleBackend
    import test_gpu_commit_open as CO
    from test_gpu_excess_keys import _s_of, _with_s
    key = (name, None)
    st, _, triples, _, files = CO._case(ec, name)
    be, binary, nr = OracleBackend(ec), name == "bin_test", len(st.rds)
    rng = random.Random("poisoned block %s %d" % (name, salt))
    _, _, Bp = RP._excess_bases(st)
    proven = host_files(key, js)
    coms, proofs = [c for c, _ in proven] + [files[r] for r in rows], [p for _, p in proven]
    prows = [_rows(ec, key, j) for j in js]
    flat_t = [((r[0], 0, r[1]) if binary else tuple(r)) for row in prows for r in row] + [t for r in rows for t in triples[r]]
    flat_p = [p for c in coms for p in E.decode_commitments(nr, c, Lift(ec).many)[0]]
    npr, total = len(js) * nr, len(flat_t)
    ss, en, ks, xs, claims = [0], [], [0], [], []
    for t, (ne, nk) in enumerate([(4, 1), (3, 2), (2, 0)]):
        picks = [(rng.randrange(npr), False), (npr + rng.randrange(total - npr), True)] + [(rng.randrange(total), rng.random() < 0.5) for _ in range(ne - 2)]
        mine_en = [RP.tally_entry(j, sub) for j, sub in picks]
        en += mine_en
        ss.append(len(en))
        a, ty, e = RP.tally_claims_host(flat_t, [0, ne], mine_en)[0]
        mine = [rng.randrange(1, N) for _ in range(nk)]
        xs += mine
        ks.append(len(xs))
        claims.append((a, ty, (e - sum(mine)) % N))
    msgs = [hashlib.sha256(b"poisoned block msg %d %d" % (salt, k)).digest() for k in range(len(xs))]
    signed = [RP.excess_sign_host(be, st, x, mg, AUX) for x, mg in zip(xs, msgs)]
    keys, sigs = [RP.excess_key33(s[2]) for s in signed], [s[1] for s in signed]
    malf = [False] * 3
    if wrong:
        p = bytearray(proofs[1]); p[10] ^= 1; proofs[1] = bytes(p)
        sigs[0] = _with_s(sigs[0], (_s_of(sigs[0]) + 1) % N)
        claims[0] = ((claims[0][0] + 1) % N,) + claims[0][1:]
        m = en[ss[2] + 1] & MASK                                    # the unproven row's commitment of sum 2
        assert m >= npr
        coms[m // nr] = CO._set_x(coms[m // nr], nr, m % nr, CO._no_point_x(ec))
        malf = [any(e & MASK == m for e in en[ss[t]:ss[t + 1]]) for t in range(3)]
    S = RP.tally_sums(be, flat_p, ss, en)
    cut = (lambda c: (c[0], c[2])) if binary else (lambda c: tuple(c))
    want_p = [INVALID if wrong and b == 1 else VALID for b in range(len(js))]
    want_k = [RP.excess_verify_key_host(be, st, k, mg, sg) for k, mg, sg in zip(keys, msgs, sigs)]
    want_s = [RP.excess_sums_host(be, st, S[t], cut(claims[t]), keys[ks[t]:ks[t + 1]], malformed=malf[t])[0] for t in range(3)]
    if wrong:
        assert want_k[0] == MISMATCH and want_s[2] == MALFORMED and MISMATCH in want_s
    else:
        assert want_k == [OK] * len(keys) and want_s == [OK] * 3
    args = (coms, proofs, ss, en, [cut(x) for x in claims], ks, keys, msgs, sigs)
    return args, [not wrong, [want_p, want_k, want_s], None]


@pytest.mark.parametrize("device", [False, True])
def test_block_call_after_poison(gpu, oracle_lib, device):
    for name in BAL_NAMES:
        nat = _native(gpu, oracle_lib, (name, None), host_oracle_max=0, **COMB)
        _chunks(nat, 12, tally=16)                                  # a block is ONE pass by contract (csrc/rpblock.hip refuses a longer one): its 9 entries + 3 keys and its 3 keys just fit
        try:
            steps = []
            for js, rows, salt, wrong in (((30, 31, 32, 33), list(range(0, 8)), 1, True), ((34, 35, 36, 37), list(range(8, 16)), 2, False),
                                          ((38, 39, 40, 41), list(range(16, 24)), 3, True), ((42, 43), list(range(24, 27)), 4, True), ((44, 45), list(range(27, 30)), 5, False)):
                args, want = _block_job(oracle_lib, name, js, rows, salt, wrong)
                fn = nat.verify_block_device if device else nat.verify_block
                steps.append(((lambda fn, args: lambda: _plain(fn(*args, seed=BAL_SEED, want_status=True)))(fn, args), want))
            sequence(steps, [gpu], [nat])
        finally:
            nat.close()
