"""The setups at the native layer's size-class edges (tests/schema_sweep.py size_edges) on the CPU: what the list covers — base-map slots,
reciprocal-table classes, reciprocal symbols, the side of every LDS edge by the launches' own planning functions
(bppp_test_rp_lds_plan, which needs no GPU) —, that bppp_rp_shape_of refuses what bppp_rp_create refuses, and that the host protocol code
proves and verifies every member the native layer accepts (and the 17-base setup, which it refuses).
tests/test_gpu_size_classes.py compares the native layer with the host code on each."""
import ctypes as C

import pytest

import pyoracle as O
import schema_sweep as SW
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from test_few_rounds_host import PointBackend

N = O.N
EDGES = SW.size_edges()
NAMES = [s.name for s in EDGES]
RECIPROCAL = [s for s in EDGES if not s.binary]
REPICK = "the launch formulas moved: pick the shapes of schema_sweep.size_edges() again"


def _setup(s):
    return SW.host_setup(RP.Backend(), s)


def symbols(st):
    """the reciprocal symbols as csrc/rp.hip numbers them: the distinct values among the digits of every inline range and shared base, and the
    public amounts' types"""
    vals = set()
    for rd in st.rds:
        if not rd.is_assumed and not rd.is_shared:
            vals |= set(range(1, rd.base)) | ({1} if rd.has_bit else set())
    for b in st.m_bases:
        vals |= set(range(1, b))
    return vals | {ty % N for _, ty, _ in st.pub_vt}


def table_class(st):
    t = 16
    while t < max(rd.base for rd in st.rds if not rd.is_assumed):
        t *= 2
    return t


def lds_class(nbytes):
    return "default" if nbytes <= SW.LDS_DEFAULT else "above" if nbytes <= SW.LDS_MAX else "over"


def planned(s, st):
    """(lds2, lds3, public) classes of a reciprocal setup by the planning hook, as size_expect names them"""
    nr, widest = len(st.rds), max(rd.base for rd in st.rds if not rd.is_assumed)
    p2, p3 = SW.lds_plan(SW.K_PHASE2, widest, nr), SW.lds_plan(SW.K_PHASE3, widest, nr)
    pub = SW.lds_plan(SW.K_PUBLIC, 0, nr, len(symbols(st)), 3)
    assert p2.table == table_class(st) and (p2.fits, p3.fits) == (int(p2.lds_bytes <= SW.LDS_MAX), int(p3.lds_bytes <= SW.LDS_MAX)) and p2.lanes == pub.lanes == 64
    assert pub.split == int(not pub.fits)                          # a small batch takes the three kernels only where one does not fit
    return lds_class(p2.lds_bytes), lds_class(p3.lds_bytes), "three" if pub.split else lds_class(pub.lds_bytes)


def test_the_list_is_deterministic_and_apart_from_the_sweep():
    assert [s.name for s in SW.size_edges()] == NAMES and SW.size_edges() == EDGES
    assert all(n.startswith("size-") for n in NAMES) and not any(s.name.startswith("size-") for s in SW.sweep() + SW.edge_setups())
    assert all(SW.by_name(n).name == n for n in NAMES) and SW.by_name(SW.sweep()[0].name) == SW.sweep()[0]
    assert (SW.MAX_NRM, SW.MAX_LIN, SW.N_RECIPROCAL, SW.N_BINARY, len(SW.points())) == (48, 40, 32, 12, 108)
    for s in EDGES:
        rows = SW._rows_of(s.ranges, s.binary)
        assert len(s.wits) == 3 and s.flavour in ("NL", "IP")
        for k, wit in enumerate(s.wits):
            assert all(asm or lo <= v <= hi1 for (_, lo, hi1, asm), v in zip(rows, wit))
            if s.cons:
                assert s.net_public + sum(sg * v for (sg, _, _, _), v in zip(rows, wit)) == 0
            elif k < 2:                                            # untyped: every range at its minimum, then at max - 1
                assert all(v == (lo if k == 0 else hi1) for (_, lo, hi1, _), v in zip(rows, wit))
    assert [s.flavour for s in EDGES].count("IP") == 1


def test_the_planning_hook_is_the_launch_formulas_edge_by_edge():
    """the counts found by bisection sit exactly on their edges, and the hook refuses nonsense"""
    e = SW.lds_edges()
    for key, kernel, limit in (("phase2_64k", SW.K_PHASE2, SW.LDS_DEFAULT), ("phase3_64k", SW.K_PHASE3, SW.LDS_DEFAULT)):
        assert SW.lds_plan(kernel, 2, e[key] - 1).lds_bytes <= limit < SW.lds_plan(kernel, 2, e[key]).lds_bytes
    assert SW.lds_plan(SW.K_PUBLIC, 0, e["public_64k"] - 1, 1, 1).lds_bytes <= SW.LDS_DEFAULT < SW.lds_plan(SW.K_PUBLIC, 0, e["public_64k"], 1, 1).lds_bytes
    assert SW.lds_plan(SW.K_PHASE2, 2, e["phase2_max"]).fits == 1 and SW.lds_plan(SW.K_PHASE2, 2, e["phase2_max"] + 1).fits == 0
    at, past = SW.lds_plan(SW.K_PUBLIC, 0, e["public_max"], 1, 1), SW.lds_plan(SW.K_PUBLIC, 0, e["public_max"] + 1, 1, 1)
    assert (at.fits, at.split, past.fits, past.split) == (1, 0, 0, 1)
    # nsyms + nr is what counts for k_trrp_public; a batch above 1024 proofs takes the three kernels whatever the setup
    assert SW.lds_plan(SW.K_PUBLIC, 0, e["public_max"] - 10, 11, 1).lds_bytes == at.lds_bytes
    assert SW.lds_plan(SW.K_PUBLIC, 0, 4, 3, 1024).split == 0 and SW.lds_plan(SW.K_PUBLIC, 0, 4, 3, 1025).split == 1
    # the table classes: a power of two at or above the widest base, 16 at the least
    assert [SW.lds_plan(SW.K_PHASE2, b, 1).table for b in (2, 16, 17, 256, 257, 512, 513, 1023)] == [16, 16, 32, 256, 512, 512, 1024, 1024]
    r = capi.TestRpLdsPlan()
    tl = capi.load_test_library()
    assert tl.bppp_test_rp_lds_plan(1, 2, 4, 1, 1, C.byref(r)) != 0 and tl.bppp_test_rp_lds_plan(SW.K_PUBLIC, 0, 4, 1, 0, C.byref(r)) != 0
    assert tl.bppp_test_rp_lds_plan(SW.K_PHASE2, 2, 4, 1, 1, None) != 0


@pytest.mark.parametrize("name", [s.name for s in RECIPROCAL])
def test_every_member_sits_in_the_class_it_was_built_for(name):
    s, e = SW.by_name(name), SW.size_expect(name)
    st = _setup(s)
    assert len(st.sorted_bases) == e["slots"], REPICK
    assert len(symbols(st)) == e["nsyms"], REPICK
    if e["refused"]:
        assert len(st.sorted_bases) > SW.MAX_SLOTS or len(symbols(st)) > SW.MAX_SYMS
        return
    assert len(st.sorted_bases) <= SW.MAX_SLOTS and len(symbols(st)) <= SW.MAX_SYMS
    assert table_class(st) == e["table"], REPICK
    assert planned(s, st) == (e["lds2"], e["lds3"], e["public"]), REPICK
    # the route of a default prove: the host algebra where a phase does not fit, or a table wider than 256 meets more than 256 ranges
    host = "over" in (e["lds2"], e["lds3"]) or (e["table"] > 256 and len(st.rds) > 256)
    assert e["prove"] == ("host" if host else "device"), REPICK


def test_what_the_classes_cover():
    exp = {s.name: SW.size_expect(s.name) for s in EDGES}
    sts = {s.name: _setup(s) for s in RECIPROCAL}
    ok = [s for s in RECIPROCAL if not exp[s.name]["refused"]]
    # a: every slot of the base map, a shared and an inline range among slots 12 .. 15, no leading bit; typed and IP once each
    a = [s for s in ok if s.name.startswith("size-a-")]
    assert len(a) == 3 and {(s.cons, s.flavour) for s in a} == {(False, "NL"), (True, "NL"), (False, "IP")}
    for s in a:
        st = sts[s.name]
        assert st.sorted_bases == list(range(2, 18)) and not any(rd.has_bit for rd in st.rds)
        high = [rd for rd in st.rds if st.sorted_bases.index(rd.base) >= 12]
        assert {rd.is_shared for rd in high} == {False, True}
        assert st.sorted_bases.index(17) == 15 and any(rd.base == 17 for rd in high)
    assert any(len(s.pubs) >= 3 for s in a if s.cons)
    b = SW.by_name("size-b-bases17-untyped-NL")
    assert sts[b.name].sorted_bases == list(range(2, 19)) and b.ranges[:16] == a[0].ranges
    # c: both sides of every table class edge, each with a digit equal to base - 1 in the second row (the table's last live entry)
    c = [s for s in ok if s.name.startswith("size-c-") and s.name.endswith("-shared")]
    assert sorted((s.ranges[0][0], exp[s.name]["table"]) for s in c) == [(16, 16), (17, 32), (256, 256), (257, 512), (512, 512), (513, 1024), (1023, 1024)]
    for s in c:
        rd = SW.range_data(s)[0]
        assert rd.is_shared and len(rd.base_coeffs) == 1 and RP.digits(rd, s.wits[1][0] - rd.lo) == [rd.base - 1] and s.ranges[1][0] == 4
    assert {exp[s.name]["table"] for s in ok} >= {16, 32, 256, 512, 1024}
    # an assumed range whose base is far above the table class of the live ranges: it has no coefficients, so no digit and no symbol
    asm = SW.by_name("size-c-base4-beside-assumed-base2000")
    assert [(r[0], r[5]) for r in asm.ranges] == [(4, False), (2000, True)] and exp[asm.name]["table"] == 16 and exp[asm.name]["prove"] == "device"
    assert SW.range_data(asm)[1].base_coeffs == [] and sts[asm.name].sorted_bases == [4] and sts[asm.name].m_bases == [4]
    # d: the symbol limit from both sides, by a base alone and by public types
    assert max(exp[s.name]["nsyms"] for s in ok) == SW.MAX_SYMS and sum(exp[s.name]["nsyms"] == SW.MAX_SYMS for s in ok) == 2
    over = [s for s in RECIPROCAL if exp[s.name]["refused"] and exp[s.name]["nsyms"] > SW.MAX_SYMS]
    assert sorted((exp[s.name]["nsyms"], len(s.pubs) > 0) for s in over) == [(SW.MAX_SYMS + 1, False), (SW.MAX_SYMS + 1, True)]
    at = SW.by_name("size-d-base1000-typed-at-the-limit")
    assert at.cons and len({t for _, t, _ in at.pubs}) == SW.MAX_SYMS - 999 and sts[at.name].m_bases == [1000]
    # a public type that is also a digit shares its symbol (the typed member of a: types 15 and 7 beside the digits 1 .. 16)
    typed_a = next(s for s in a if s.cons)
    assert {t for _, t, _ in typed_a.pubs} & set(range(1, 17)) and exp[typed_a.name]["nsyms"] == 16
    # e: the prover's wide-table clause from both sides
    assert [(len(s.ranges), exp[s.name]["table"], exp[s.name]["prove"]) for s in ok if s.name.startswith("size-e-")] == [(256, 512, "device"), (257, 512, "host")]
    # f, g, h: every 64 KiB edge from both sides, the two 160 KiB limits from both sides
    assert {exp[s.name]["lds3"] for s in ok if s.name.startswith("size-f-")} == {"default", "above"}
    assert all((exp[s.name]["lds2"], exp[s.name]["public"]) == ("above", "above") for s in ok if s.name.startswith("size-f-"))
    assert any(s.cons for s in ok if s.name.startswith("size-f-"))
    assert {exp[s.name]["lds2"] for s in ok} == {"default", "above", "over"} and {exp[s.name]["public"] for s in ok} == {"default", "above", "three"}
    g = [s for s in ok if s.name.startswith("size-g-")]
    h = [s for s in ok if s.name.startswith("size-h-")]
    assert [(exp[s.name]["lds2"], exp[s.name]["prove"]) for s in g] == [("above", "device"), ("over", "host")] and len(g[1].ranges) == len(g[0].ranges) + 1
    assert [exp[s.name]["public"] for s in h] == ["above", "three"] and len(h[1].ranges) == len(h[0].ranges) + 1
    # i: the binary range limit from both sides
    i = [s for s in EDGES if s.binary]
    assert [(len(s.ranges), bool(exp[s.name]["refused"]), s.cons) for s in i] == [(1024, False, True), (1025, True, True)]
    assert all(hi - lo == 2 for s in i for lo, hi, _, _ in s.ranges)


def _ranges_array(st):
    arr = (capi.RpRange * len(st.rds))()
    for r, rd in zip(arr, st.rds):
        r.base = rd.base
        r.flags = (capi.RP_SHARED if rd.is_shared else 0) | (capi.RP_OUTPUT if rd.is_output else 0) | (capi.RP_ASSUMED if rd.is_assumed else 0)
        r.min[:] = [int(v) for v in capi.int_to_limbs(rd.lo % 2**256)]
        r.max[:] = [int(v) for v in capi.int_to_limbs(rd.hi % 2**256)]
    return arr


def shape_of(st):
    """bppp_rp_shape_of (host only): (rc, shape)"""
    lib = capi.load_library()
    shp = capi.RpShape()
    rc = lib.bppp_rp_shape_of(0 if st.flavour == "NL" else 1, int(st.has_types), C.cast(_ranges_array(st), C.c_void_p), len(st.rds), C.byref(shp))
    return rc, shp


@pytest.mark.parametrize("name", [s.name for s in RECIPROCAL])
def test_shape_of_refuses_what_create_refuses(name):
    """bppp_rp_shape_of knows the ranges, not the public amounts: it refuses the 17th base and the base of 1024 and reports the host setup's
    shape for everything else (the member refused for its public TYPES is a matter of bppp_rp_create alone)"""
    s, e = SW.by_name(name), SW.size_expect(name)
    st = _setup(s)
    rc, shp = shape_of(st)
    if e["refused"] and not s.pubs:
        assert rc == -1
        return
    assert rc == 0
    assert (shp.nranges, shp.norm_len, shp.lin_len, shp.rounds, (shp.final_norm, shp.final_lin)) == (len(st.rds), st.nrm_len, st.lin_len, st.rounds, tuple(st.final_lens))


class _Ranges:
    """as much of a host setup as shape_of and _ranges_array read"""

    def __init__(self, rds, flavour="NL", has_types=False):
        self.rds, self.flavour, self.has_types = rds, flavour, has_types


def many_small_ranges(n):
    """n inline base-2 ranges of width 2: one norm position each, no basis point needed to ask for their shape"""
    return _Ranges([RP.make_range_data(2, 0, 2, False, i % 2 == 1, False) for i in range(n)])


def test_shape_of_refuses_the_65536th_range():
    """every prover route indexes ranges below 2^16, the host algebra included: 65535 ranges have a shape, 65536 have none"""
    rc, shp = shape_of(many_small_ranges(SW.MAX_RANGES))
    assert rc == 0 and (shp.nranges, shp.norm_len, shp.lin_len) == (SW.MAX_RANGES, SW.MAX_RANGES, 6)
    assert shape_of(many_small_ranges(SW.MAX_RANGES + 1))[0] == -1


def host_rows(s):
    """the witness rows the host proves: all three, or the random row alone for a setup of more than 1000 ranges (seconds a proof)"""
    return (0, 1, 2) if len(s.ranges) <= 1000 else (2,)


@pytest.mark.parametrize("name", [s.name for s in EDGES if not SW.size_expect(s.name)["refused"]] + ["size-b-bases17-untyped-NL"])
def test_honest_proofs_verify(oracle_lib, name):
    s = SW.by_name(name)
    mod = BRP if s.binary else RP
    be = PointBackend(oracle_lib)
    st = SW.host_setup(be, s)
    for j in host_rows(s):
        proof = SW.host_prove(st, s, j)
        assert mod.verify(st, proof, RP.sha256_oracle()) and be.last is None, j
        assert len(proof.responses) == st.rounds and (len(proof.wit_nrm), len(proof.wit_lin)) == tuple(st.final_lens)
        if len(s.ranges) <= 1000:
            assert not mod.verify(st, proof, RP.sha256_oracle(b"another oracle")) and be.last is not None
