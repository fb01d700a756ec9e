"""The setups at the native layer's size-class edges (tests/schema_sweep.py size_edges) on the GPU, with the machinery of the schema sweep
(tests/test_gpu_schema_sweep.py): per accepted setup the handle's shape, the witness kernels, the prover's bytes on four routes, the
verifier's public scalars, and verdicts and points on single-field mutations — every comparison exact against the host protocol code.

Every case also asserts, through bppp_test_rp_last_prove / bppp_test_rp_last_public / bppp_test_trrp_last_public, that it RAN in the class it
was built for (size_expect): the table class, the dynamic LDS of the phase kernels and of k_trrp_public on its side of 64 KiB, the device
or the host algebra, one kernel or three.  A launch formula that moves makes these fail with REPICK instead of passing on the wrong side.

The rule pinned for the limits: a setup that bppp_rp_create accepts never fails later for its size (past the prover's LDS limit a prove
takes the host algebra, past the verifier's the three kernels), and what it refuses — a 17th digit base, a 1023rd reciprocal symbol, a
65536th range (the host algebra's own limit), a 1025th binary range — it refuses at creation, in the caller's terms, leaving the context
usable.  What the reports cannot show is whether a launch above 64 KiB asked for its LDS with hipFuncSetAttribute: they give the bytes
planned and launched, and such a launch has been seen to run without the call.

Host time: a proof of thousands of ranges takes the host protocol code seconds, so setups above 1000 ranges prove one witness row (the
random one) instead of three, and setups above 64 ranges verify the first and the last mutation of every field family (asserted on the
list) instead of all of them.  tests/test_size_classes_host.py pins what the list covers."""
import ctypes as C
import random

import numpy as np
import pytest

import pyoracle as O
import schema_sweep as SW
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import BpppError
from test_gpu_schema_sweep import (Case, _check_public_rows, _refused_rows, check_prover_bytes, check_public_scalars, check_verdicts_and_points,
                                   check_witness_kernel)
from test_size_classes_host import REPICK, _ranges_array, host_rows, many_small_ranges, shape_of

pytestmark = pytest.mark.gpu

N = O.N
EDGES = SW.size_edges()
ACCEPTED = [s.name for s in EDGES if not SW.size_expect(s.name)["refused"]]
ACCEPTED_RECIPROCAL = [s.name for s in EDGES if not SW.size_expect(s.name)["refused"] and not s.binary]
REFUSED = [s.name for s in EDGES if SW.size_expect(s.name)["refused"]]
SPLIT_BATCH = [n for n in ACCEPTED_RECIPROCAL if n.startswith(("size-f-", "size-h-"))]
DEVICE_ALGEBRA, HOST_ALGEBRA = capi.TEST_RP_PROVE_DEVICE_ALGEBRA, capi.TEST_RP_PROVE_HOST_ALGEBRA
ONE_KERNEL, THREE_KERNELS = capi.TEST_RP_PUBLIC_ONE_KERNEL, capi.TEST_RP_PUBLIC_THREE_KERNELS

_CASES = {}


def _case(ec, name):
    if name not in _CASES:
        _CASES[name] = Case(ec, name, host_rows(SW.by_name(name)))
    return _CASES[name]


# ----------------------------------------------------------------------------- what ran
def _last_prove(nat):
    r = capi.TestRpProveReport()
    nat.gpu._check(capi.load_test_library().bppp_test_rp_last_prove(nat.h, C.byref(r)), "bppp_test_rp_last_prove")
    return r


def _last_public(gpu, handle, tables=False):
    r = capi.TestRpPublicReport()
    tl = capi.load_test_library()
    gpu._check((tl.bppp_test_trrp_last_public if tables else tl.bppp_test_rp_last_public)(handle, C.byref(r)), "bppp_test_rp_last_public")
    return r


def _in_class(nbytes, cls):
    return {"default": 0 < nbytes <= SW.LDS_DEFAULT, "above": SW.LDS_DEFAULT < nbytes <= SW.LDS_MAX}[cls]


def _assert_public_class(r, e, nsyms_nr):
    """a batch of at most 1024 proofs: k_trrp_public with a wavefront per proof on its side of 64 KiB, or the three kernels"""
    if e["public"] == "three":
        assert (r.route, r.lanes, r.lds_bytes) == (THREE_KERNELS, 0, 0), REPICK
        return
    assert r.route == ONE_KERNEL and r.lanes == 64 and _in_class(r.lds_bytes, e["public"]), (REPICK, r.route, r.lanes, r.lds_bytes)
    assert r.lds_bytes == SW.lds_plan(SW.K_PUBLIC, 0, nsyms_nr[1], nsyms_nr[0], 1).lds_bytes


def _assert_prove_class(nat, e, route):
    """the route and the LDS of the prove that just ran; `route` names what check_prover_bytes asked for"""
    r = _last_prove(nat)
    nr = len(nat.st.rds)
    assert r.table == e["table"], REPICK
    # the inner-product flavour has its device algebra over the comb table only: its first prove, before the table, is the host algebra's
    no_table_yet = nat.st.flavour == "IP" and route == "default"
    want = HOST_ALGEBRA if route == "host algebra" or e["prove"] == "host" or no_table_yet else DEVICE_ALGEBRA
    assert r.route == want, (REPICK, route, r.route)
    if want == HOST_ALGEBRA:
        assert (r.lds2_bytes, r.lds3_bytes) == (0, 0)
        return
    assert _in_class(r.lds2_bytes, e["lds2"]) and _in_class(r.lds3_bytes, e["lds3"]), (REPICK, r.lds2_bytes, r.lds3_bytes)
    widest = max(rd.base for rd in nat.st.rds if not rd.is_assumed)
    assert (r.lds2_bytes, r.lds3_bytes) == (SW.lds_plan(SW.K_PHASE2, widest, nr).lds_bytes, SW.lds_plan(SW.K_PHASE3, widest, nr).lds_bytes)
    _assert_public_class(_last_public(nat.gpu, nat.h), e, (e["nsyms"], nr))      # the device algebra takes its public scalars from the verifier's kernel


# ----------------------------------------------------------------------------- 1, 2. the handle's shape and the witness kernels
@pytest.mark.parametrize("name", ACCEPTED)
def test_setup_and_witness_kernel(gpu, oracle_lib, name):
    c = _case(oracle_lib, name)
    nat = c.native(gpu)                                            # asserts the host setup's shape
    try:
        live = [i for i, r in enumerate(c.s.ranges) if not r[-1]]
        refused = _refused_rows(c, {live[0], live[-1]}) if len(c.s.ranges) > 64 else None
        check_witness_kernel(c, nat, refused)
        if not c.s.binary:                                         # bppp_rp_shape_of agrees with the handle
            rc, shp = shape_of(c.st)
            assert rc == 0 and {n: int(getattr(shp, n)) for n, _ in capi.RpShape._fields_} == nat.shape
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 3. the prover's bytes on four routes, each in its class
@pytest.mark.parametrize("name", ACCEPTED)
def test_prover_writes_the_host_protocols_bytes(gpu, oracle_lib, name):
    c, e = _case(oracle_lib, name), SW.size_expect(name)
    nat = c.native(gpu)
    try:
        routes = []

        def after(route):
            routes.append(route)
            if not c.s.binary:
                _assert_prove_class(nat, e, route)
        check_prover_bytes(c, nat, after)
        assert routes == ["default", "comb device hash", "comb host hash", "host algebra"]
    finally:
        nat.close()


# ----------------------------------------------------------------------------- 4. the verifier's public scalars
@pytest.mark.parametrize("name", ACCEPTED_RECIPROCAL)
def test_device_derived_verifier_scalars_equal_the_host_derivation(gpu, oracle_lib, name):
    c, e = _case(oracle_lib, name), SW.size_expect(name)
    tabs = RP.DeviceVerifierTables(gpu, c.st)
    try:
        assert _last_public(gpu, tabs.h, True).route == 0
        check_public_scalars(c, tabs, name)
        _assert_public_class(_last_public(gpu, tabs.h, True), e, (e["nsyms"], len(c.st.rds)))
    finally:
        tabs.close()


def _public_arrays(tabs, ch):
    """bppp_trrp_public_device on challenges given as a [B * 7][4] array: the five outputs as arrays (no conversion to integers)"""
    gpu, st, B = tabs.gpu, tabs.st, ch.shape[0] // 7
    sizes = {"q": B, "sp": B, "pub_norm": B * st.nrm_len, "pub_lin_c": B * st.lin_len, "init_scalars": B * tabs.ninit}
    d_ch = gpu.to_device(ch)
    bufs = {k: gpu.to_device(np.zeros((n, 4), dtype=np.uint64)) for k, n in sizes.items()}
    try:
        tabs.public_device(B, d_ch, bufs["q"], bufs["sp"], bufs["pub_norm"], bufs["pub_lin_c"], bufs["init_scalars"])
        return {k: gpu.download(bufs[k], (n, 4)) for k, n in sizes.items()}
    finally:
        gpu.free(d_ch)
        for p in bufs.values():
            gpu.free(p)


@pytest.mark.parametrize("name", SPLIT_BATCH)
def test_public_scalars_1100_rows_equal_two_batches_of_550(gpu, oracle_lib, name):
    """1100 rows run as the three kernels whatever the setup; 550 rows as the one kernel while its LDS fits: identical outputs, and rows of
    them equal the host derivation"""
    c, e = _case(oracle_lib, name), SW.size_expect(name)
    st = c.st
    tabs = RP.DeviceVerifierTables(gpu, st)
    try:
        rnd = random.Random("size classes split " + name)
        ch = np.frombuffer(rnd.randbytes(1100 * 7 * 32), dtype=np.uint64).reshape(-1, 4).copy()
        ch[:, 3] >>= np.uint64(1)                                  # below 2^255: canonical
        ch[7 * 7:8 * 7] = capi.scalars_to_array([1, 2, 3, 4, 5, 6, 7]); ch[1099 * 7:] = capi.scalars_to_array([N - 1] * 7)
        big = _public_arrays(tabs, ch)
        assert _last_public(gpu, tabs.h, True).route == THREE_KERNELS
        halves = [_public_arrays(tabs, ch[:550 * 7]), _public_arrays(tabs, ch[550 * 7:])]
        _assert_public_class(_last_public(gpu, tabs.h, True), e, (e["nsyms"], len(st.rds)))
        for k, a in big.items():
            assert np.array_equal(a, np.concatenate([h[k] for h in halves])), k
        rows = (0, 7, 600, 1099)
        per = {"q": 1, "sp": 1, "pub_norm": st.nrm_len, "pub_lin_c": st.lin_len, "init_scalars": tabs.ninit}
        got = []
        for b in rows:
            cut = {k: capi.array_to_scalars(big[k][b * n:(b + 1) * n]) for k, n in per.items()}
            got.append(dict(cut, q=cut["q"][0], sp=cut["sp"][0]))
        _check_public_rows(st, c.proofs[0].coms, [capi.array_to_scalars(ch[7 * b:7 * b + 7]) for b in rows], got)
    finally:
        tabs.close()


# ----------------------------------------------------------------------------- 5. verdicts and points
def field_families(L):
    """the labels of test_gpu_few_rounds._mutants by field family, in order"""
    fam = {"input commitments": ["sign of input commitment %d" % i for i in range(L.nr)],
           "round points": ["sign of proof point %d" % i for i in range(L.nrp, L.npp)],
           "final norm scalars": ["scalar %d" % i for i in range(L.fn)], "final linear scalars": ["scalar %d" % i for i in range(L.fn, L.ns)]}
    for j in range(L.nrp):
        fam["range-proof commitment %d" % j] = ["sign of proof point %d" % j]
    return {k: v for k, v in fam.items() if v}


EXCHANGES = ["points 0 and 1 exchanged", "the last two points exchanged"]


def pick_mutants(L, ms):
    """every mutation up to 64 ranges; beyond, the first and the last member of every field family and the two exchanges — checked on the list"""
    fam = field_families(L)
    labels = [m[0] for m in ms]
    assert sorted(labels) == sorted([x for v in fam.values() for x in v] + EXCHANGES)       # _mutants makes these families and nothing else
    if L.nr <= 64:
        return ms
    keep = {v[0] for v in fam.values()} | {v[-1] for v in fam.values()} | set(EXCHANGES)
    picked = [m for m in ms if m[0] in keep]
    have = {m[0] for m in picked}
    for k, v in fam.items():
        assert v[0] in have and v[-1] in have, k
    return picked


@pytest.mark.parametrize("name", ACCEPTED)
def test_verdicts_and_points_on_single_field_mutations(gpu, oracle_lib, name):
    c, e = _case(oracle_lib, name), SW.size_expect(name)
    nat = c.native(gpu)
    try:
        check_verdicts_and_points(gpu, oracle_lib, c, nat, pick_mutants)
        if not c.s.binary:                                         # the verifications ran k_trrp_public (or the three kernels) in the setup's class
            _assert_public_class(_last_public(gpu, nat.h), e, (e["nsyms"], len(c.st.rds)))
    finally:
        nat.close()


# ----------------------------------------------------------------------------- refused at creation, in the caller's terms
@pytest.mark.parametrize("name", REFUSED)
def test_refused_at_creation_and_the_context_stays_usable(gpu, name):
    s, e = SW.by_name(name), SW.size_expect(name)
    st = SW.host_setup(RP.Backend(), s)
    entry = "bppp_rp_create_binary" if s.binary else "bppp_rp_create"
    for _ in range(2):                                             # the second refusal finds the context as the first left it
        with pytest.raises(BpppError) as err:
            (BRP.NativeBinaryRangeProofs if s.binary else RP.NativeRangeProofs)(gpu, st).close()
        assert entry + " failed (-1)" in str(err.value)
        for piece in e["refused"]:
            assert piece in str(err.value), (piece, str(err.value))
    if not s.binary and not s.pubs:                                # bppp_rp_shape_of refuses the same ranges
        assert shape_of(st)[0] == -1
    # a following create on the same context works, and proves
    ok = SW.edge_setups()[0]
    st_ok = SW.host_setup(RP.Backend(), ok)
    nat = RP.NativeRangeProofs(gpu, st_ok)
    try:
        files = nat.prove_batch([SW.inputs_of(ok, ok.wits[2], 2)], [SW.prefix_of(2)])
        assert nat.verify_batch([files[0][0]], [files[0][1]], b"\x05" * 32)
    finally:
        nat.close()


def test_the_65536th_range_is_refused_at_creation(gpu):
    """every prover route, the host algebra included, indexes ranges below 2^16: bppp_rp_create refuses one range more, before it looks at the
    basis (two points are given), as bppp_rp_shape_of does; the same call with 65535 ranges gets as far as counting the basis points"""
    pts = capi.points_to_array(SW.points()[:2])
    for n, pieces in ((SW.MAX_RANGES + 1, ["%d ranges" % (SW.MAX_RANGES + 1), "at most %d" % SW.MAX_RANGES]), (SW.MAX_RANGES, ["not enough basis points"])):
        st = many_small_ranges(n)
        hnd = C.c_void_p()
        rc = gpu.lib.bppp_rp_create(gpu.h, 0, 0, C.cast(_ranges_array(st), C.c_void_p), n, None, 0, C.c_void_p(pts.ctypes.data), 2, None, C.byref(hnd))
        msg = gpu.lib.bppp_last_error(gpu.h).decode()
        assert rc == -1 and not hnd.value and all(p in msg for p in pieces), msg
    assert shape_of(many_small_ranges(SW.MAX_RANGES + 1))[0] == -1
