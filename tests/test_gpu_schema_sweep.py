"""The seeded schema sweep (tests/schema_sweep.py) on the GPU: per generated setup, the native range-proof layer against the host protocol
code over the CPU oracle — every comparison exact.

 1. setup: bppp_rp_create / bppp_rp_create_binary accepts it and reports the host setup's shape;
 2. witness kernels (csrc/rpwitness.hip.h through bppp_test_rp_witness_device): scalars, digits, multiplicities and shared counts of the
    three witnesses; one range at a time at min - 1 and at max, and an unbalanced row, refused with the status of the host's refusal;
 3. prover: prove_batch writes the bytes of the host protocol's proofs on the default route, over a comb table hashing on the device and on
    the host cores, and on the host-algebra route;
 4. verifier scalars (reciprocal): bppp_trrp_public_device equals verify_rp's derivation on real, random and edge challenges;
 5. verdicts and points: the honest proof and every single-field mutation of it through verify_batch, verify_each and the combined point.

The widths below the digit base (schema_sweep.NARROW) are refused by bppp_rp_create, shared and inline; the first two widths beside them
(schema_sweep.edge_setups) go through 1 to 5 like the generated ones.  tests/test_schema_sweep_host.py pins what the list covers."""
import dataclasses
import random

import pytest

import pyoracle as O
import schema_sweep as SW
from bulletproofspp_amd import encoding as E
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import BpppError, RP_WIT_BIN_UNBALANCED, RP_WIT_OK, RP_WIT_OUT_OF_RANGE, RP_WIT_UNBALANCED
from test_few_rounds_host import PointBackend
from test_gpu_decode_conformance import Layout, Lift
from test_gpu_few_rounds import _mutants
from test_gpu_prove_device import _witness_device, _witness_host
from test_gpu_verify_each import SEED, _batch_full, _rho

pytestmark = pytest.mark.gpu

N = O.N
VALID, INVALID = 0, 1
NAMES = [s.name for s in SW.sweep() + SW.edge_setups()]
RECIPROCAL = [s.name for s in SW.sweep() + SW.edge_setups() if not s.binary]
REFUSALS = {"value outside its range": RP_WIT_OUT_OF_RANGE, "amounts of some type do not balance": RP_WIT_UNBALANCED,
            "binary witness needs a conserved schema whose amounts balance (Binary.hs:162-164)": RP_WIT_BIN_UNBALANCED}


# ----------------------------------------------------------------------------- one setup: host side once, a native handle per test
class Case:
    def __init__(self, ec, name, proved=(0, 1, 2)):
        """proved: the witness rows the host proves (all three in the sweep; a setup of thousands of ranges proves one)"""
        self.s = s = SW.by_name(name)
        self.mod = BRP if s.binary else RP
        self.nrp = 2 if s.binary else 4
        self.st = SW.host_setup(PointBackend(ec), s)
        self.inputs = [SW.inputs_of(s, w, j) for j, w in enumerate(s.wits)]
        self.proved = list(proved)
        self.p_inputs = [self.inputs[j] for j in self.proved]
        self.prefixes = [SW.prefix_of(j) for j in self.proved]
        self.proofs = [SW.host_prove(self.st, s, j) for j in self.proved]
        self.files = [E.encode_proof(self.nrp, p) for p in self.proofs]

    def native(self, gpu):
        nat = (BRP.NativeBinaryRangeProofs if self.s.binary else RP.NativeRangeProofs)(gpu, self.st)
        st = self.st
        assert (nat.shape["nranges"], nat.shape["norm_len"], nat.shape["lin_len"], nat.shape["rounds"], (nat.shape["final_norm"], nat.shape["final_lin"])) == \
            (len(st.rds), st.nrm_len, st.lin_len, st.rounds, tuple(st.final_lens))
        return nat


_CASES = {}


def _case(ec, name):
    if name not in _CASES:
        _CASES[name] = Case(ec, name)
    return _CASES[name]


# ----------------------------------------------------------------------------- 1, 2. setup and witness kernels
def _with_public(c, st, delta):
    """(`st` with its public amounts moved by `delta` in the ranges' type, the hook's per-proof public argument for it); (st, None) where
    the setup has no public amount to move"""
    s = c.s
    if s.binary:
        return dataclasses.replace(st, net_public=st.net_public + delta), st.net_public + delta
    k = next((k for k, (_, ty, _) in enumerate(s.pubs) if ty == s.ty), None)
    if k is None:
        return st, None
    io, ty, v = s.pubs[k]
    pubs = list(s.pubs)
    pubs[k] = (io, ty, (v - delta if io else v + delta) % N)
    return dataclasses.replace(st, pub_vt=pubs), [v_ for _, _, v_ in pubs]


def _host_status(c, st1, row):
    try:
        c.mod.witness(st1, row)
    except ValueError as e:
        return REFUSALS[str(e)]
    return RP_WIT_OK


def _refused_rows(c, only=None):
    """[(what, row, host setup of that row, the hook's public argument, moved)]: every live range (of the ranges `only`, if given) at min - 1 and
    at max — the balance kept through the public amount or an assumed range where the setup has one (`moved`), so that the range check is what
    refuses — and one unbalanced row"""
    s, st = c.s, c.st
    base = c.inputs[2]
    rows_of = SW._rows_of(s.ranges, s.binary)
    assumed = next((i for i, r in enumerate(rows_of) if r[3]), None)
    out = []

    def put(row, i, v):
        row = list(row)
        row[i] = (v,) + tuple(row[i][1:])
        return row

    for i, (sg, lo, hi1, asm) in enumerate(rows_of):
        if asm or (only is not None and i not in only):
            continue
        for what, v in (("range %d at min - 1" % i, lo - 1), ("range %d at max" % i, hi1 + 1)):
            delta = sg * (v - base[i][0])                          # what the signed sum of the amounts gains
            row, st1, pub, moved = put(base, i, v), st, None, not s.cons
            if s.cons:
                st1, pub = _with_public(c, st, -delta)
                moved = pub is not None
                if not moved and assumed is not None:
                    a_sg = rows_of[assumed][0]
                    row, moved = put(row, assumed, row[assumed][0] - a_sg * delta), True
            out.append((what, row, st1, pub, moved))
    # unbalanced: the public amount one off, else an amount one off inside its range
    if s.cons:
        st1, pub = _with_public(c, st, 1)
        if pub is not None:
            out.append(("public amount + 1", list(base), st1, pub, None))
        else:
            i, v = next((i, v) for i, (sg, lo, hi1, asm) in enumerate(rows_of) for v in (base[i][0] + 1, base[i][0] - 1) if asm or lo <= v <= hi1)
            out.append(("amount %d one off" % i, put(base, i, v), st, None, None))
    return out


def check_witness_kernel(c, nat, refused=None):
    """the witness kernels on the three rows of the case and on `refused` (default: every live range at min - 1 and at max, and an unbalanced row)"""
    s, st = c.s, c.st
    refused = _refused_rows(c) if refused is None else refused
    rows = c.inputs + [r for _, r, _, _, _ in refused]
    sts = [st] * 3 + [st1 for _, _, st1, _, _ in refused]
    own = st.net_public if s.binary else [v % N for _, _, v in s.pubs]
    pubs = None
    if s.binary or any(p is not None for _, _, _, p, _ in refused):
        pubs = [own] * 3 + [own if p is None else p for _, _, _, p, _ in refused]
    want = [_host_status(c, st1, row) for st1, row in zip(sts, rows)]
    assert want[:3] == [RP_WIT_OK] * 3
    for (what, _, _, _, moved), w in zip(refused, want[3:]):
        if moved is None:                                      # the unbalanced row
            assert w == (RP_WIT_BIN_UNBALANCED if s.binary else RP_WIT_UNBALANCED), what
        else:                                                  # a range check, unless nothing could keep the balance
            assert w == (RP_WIT_OUT_OF_RANGE if moved else RP_WIT_UNBALANCED), what
    sc, dig, mul, mss, status = _witness_device(nat, rows, pubs)
    assert status == want, [w for w, _, _, _, _ in refused]
    for b in range(3):
        if s.binary:
            assert sc[b] == [(v % N, bl % N, 0) for v, bl in rows[b]], b
            assert dig[b] == [int(d) for d in BRP.witness(st, rows[b])[1]], b
        else:
            assert (sc[b], dig[b], mul[b], mss[b]) == _witness_host(st, rows[b]), b


@pytest.mark.parametrize("name", NAMES)
def test_setup_and_witness_kernel(gpu, oracle_lib, name):
    c = _case(oracle_lib, name)
    nat = c.native(gpu)
    try:
        check_witness_kernel(c, nat)
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 3. the prover's bytes on four routes
def check_prover_bytes(c, nat, after=lambda route: None):
    """the four prover routes write the host protocol's bytes; `after(route)` is called behind each prove ("default", "comb device hash",
    "comb host hash", "host algebra")"""
    want = c.files
    assert nat.prove_batch(c.p_inputs, c.prefixes) == want
    after("default")
    nat.set_option("comb_min", 1); nat.set_option("comb_bits", 7)
    for host_oracle_max in (0, 2**64 - 1):                     # a comb table of the basis; hashing on the device, then on the host cores
        nat.set_option("host_oracle_max", host_oracle_max)
        assert nat.prove_batch(c.p_inputs, c.prefixes) == want, host_oracle_max
        after("comb host hash" if host_oracle_max else "comb device hash")
    nat.set_option("host_algebra", 1)
    assert nat.prove_batch(c.p_inputs, c.prefixes) == want
    after("host algebra")
    nat.set_option("host_algebra", 0)
    ok, status, _ = nat.verify_batch([cf for cf, _ in want], [pf for _, pf in want], SEED, want_status=True)
    assert ok and status == [VALID] * len(want)


@pytest.mark.parametrize("name", NAMES)
def test_prover_writes_the_host_protocols_bytes(gpu, oracle_lib, name):
    c = _case(oracle_lib, name)
    nat = c.native(gpu)
    try:
        check_prover_bytes(c, nat)
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 4. the verifier's public scalars
def _check_public_rows(st, coms, chs, got):
    """rows of bppp_trrp_public_device against verify_rp replayed with an oracle that returns the row's challenges"""
    pad = lambda xs, n: list(xs) + [0] * (n - len(xs))
    for ch, g_ in zip(chs, got):
        e, x, r0, q, xp, r1, t = ch
        seq = iter([[e, x, r0], [q, xp, r1], [t]])
        sbp = RP.verify_rp(st, coms, RP.Transcript(lambda cs, n: next(seq)))
        assert g_["q"] == q % N and g_["sp"] == sbp.pub.sc
        assert g_["pub_norm"] == pad(sbp.pub.nrm, st.nrm_len)
        assert g_["pub_lin_c"] == pad(sbp.cs, st.lin_len)
        by_point = {}
        for s_, p_ in sbp.init_terms:
            by_point[p_] = (by_point.get(p_, 0) + s_) % N
        assert len(by_point) == len(coms)
        assert g_["init_scalars"] == [by_point[p_] for p_ in coms]


def check_public_scalars(c, tabs, name):
    """bppp_trrp_public_device on the real challenges of the case's first proof, two random rows and the edge rows [1 .. 7], [N - 1] * 7"""
    st, proof = c.st, c.proofs[0]
    rnd = random.Random("schema sweep challenges " + name)
    real, es = RP.verifier_challenges(st, proof, RP.sha256_oracle())
    assert es == RP.verify_inputs(st, proof, RP.sha256_oracle())["es"]
    chs = [real] + [[rnd.randrange(N) for _ in range(7)] for _ in range(2)] + [[1, 2, 3, 4, 5, 6, 7], [N - 1] * 7]
    _check_public_rows(st, proof.coms, chs, tabs.public(chs))


@pytest.mark.parametrize("name", RECIPROCAL)
def test_device_derived_verifier_scalars_equal_the_host_derivation(gpu, oracle_lib, name):
    c = _case(oracle_lib, name)
    tabs = RP.DeviceVerifierTables(gpu, c.st)
    try:
        check_public_scalars(c, tabs, name)
    finally:
        tabs.close()


def _three_kernel_picks():
    rec = [s for s in SW.sweep() if not s.binary]
    typed = next(s for s in rec if s.cons and any(r[5] for r in s.ranges))
    untyped = next(s for s in rec if not s.cons and len(SW.host_setup(RP.Backend(), s).sorted_bases) >= 3)
    return [typed.name, untyped.name]


@pytest.mark.parametrize("name", _three_kernel_picks())
def test_public_scalars_three_kernel_route_equals_the_single_kernel(gpu, oracle_lib, name):
    """above 1024 proofs bppp_trrp_public_device runs as k_trrp_pre / k_trrp_pos / k_trrp_lin instead of the one k_trrp_public: 1100 rows as
    one batch and as two batches of 550 give identical outputs, and rows of it equal the host derivation"""
    c = _case(oracle_lib, name)
    st = c.st
    tabs = RP.DeviceVerifierTables(gpu, st)
    try:
        rnd = random.Random("schema sweep split " + name)
        chs = [[rnd.randrange(N) for _ in range(7)] for _ in range(1100)]
        chs[7] = [1, 2, 3, 4, 5, 6, 7]; chs[1099] = [N - 1] * 7
        big = tabs.public(chs)
        small = tabs.public(chs[:550]) + tabs.public(chs[550:])
        assert big == small
        rows = (0, 7, 600, 1099)
        _check_public_rows(st, c.proofs[0].coms, [chs[i] for i in rows], [big[i] for i in rows])
    finally:
        tabs.close()


# ----------------------------------------------------------------------------- 5. verdicts and points
def check_verdicts_and_points(gpu, oracle_lib, c, nat, pick=lambda L, ms: ms):
    """the honest first proof of the case and its single-field mutations (`pick` may choose among them) through verify_batch, verify_each and
    the combined point, against the host verifier over the CPU oracle"""
    st, mod, nrp = c.st, c.mod, c.nrp
    L = Layout(nat.shape, nrp)
    lift = Lift(oracle_lib)
    cf, pf = c.files[0]
    ms = pick(L, _mutants(L, cf, pf))
    files = [("honest", cf, pf)] + ms
    want_ok, want_pts = [], []
    for _, c_, p_ in files:                                    # the host protocol verifier over the CPU oracle, and the point it commits
        coms = E.decode_commitments(L.nr, c_, lift.many)
        proof = E.decode_proof(nrp, st.rounds, st.final_lens, coms[0], p_, lift.many)
        assert proof is not None                               # every mutation keeps the files well-formed
        want_ok.append(bool(mod.verify(st, proof, RP.sha256_oracle())))
        want_pts.append(st.backend.last)
    assert want_ok == [True] + [False] * len(ms)
    assert [e is None for e in want_pts] == want_ok
    coms_f, prfs = [c_ for _, c_, _ in files], [p_ for _, _, p_ in files]
    lead = nat.shape["challenges_per_proof"] - nat.shape["rounds"]
    for host_oracle_max in (None, 0):                          # the handle's default, then hashing on the device
        if host_oracle_max is not None:
            nat.set_option("host_oracle_max", host_oracle_max)
        ok, status, _ = nat.verify_batch(coms_f, prfs, SEED, want_status=True)
        assert not ok and status == [VALID] + [INVALID] * len(ms), host_oracle_max
        each, pts = nat.verify_each(coms_f, prfs, want_points=True)
        assert each == status and pts == want_pts, host_oracle_max
        ok2, st2, chs, comb = _batch_full(gpu, nat, coms_f, prfs)
        assert (ok2, st2) == (ok, status)
        rhos = [_rho(nat, SEED, b, chs[b][lead - 1], chs[b][lead] if nat.shape["rounds"] else 0, prfs[b]) for b in range(len(files))]
        assert comb == oracle_lib.inner_product([(r, e) for r, e in zip(rhos, want_pts) if e is not None]), host_oracle_max
        assert nat.verify_batch(coms_f[:1], prfs[:1], SEED) and nat.verify_each(coms_f[:1], prfs[:1], want_points=True) == ([VALID], [None])


@pytest.mark.parametrize("name", NAMES)
def test_verdicts_and_points_on_single_field_mutations(gpu, oracle_lib, name):
    c = _case(oracle_lib, name)
    nat = c.native(gpu)
    try:
        check_verdicts_and_points(gpu, oracle_lib, c, nat)
    finally:
        nat.close()


# ----------------------------------------------------------------------------- widths below the digit base
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("base,w", SW.NARROW)
def test_a_range_narrower_than_its_base_is_refused(gpu, base, w, shared):
    rd = RP.make_range_data(base, 0, w, shared, True, False)
    assert rd.base_coeffs == [w - base, 1]                         # the reference's formula, kept by the Python restatement
    st = RP.setup(RP.Backend(), SW.points(), False, [], [rd], "NL")
    with pytest.raises(BpppError) as err:
        RP.NativeRangeProofs(gpu, st).close()
    assert "bppp_rp_create failed (-1)" in str(err.value)
    assert "range 0: range narrower than its digit base: the reference's coefficients do not bound it" in str(err.value)
