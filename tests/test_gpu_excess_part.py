"""bppp_rp_excess_part_nonces*, _part_aggregate*, _part_sign*, _part_verify*, _part_combine*: builders who each know a part of the blinding sum produce
together the 65 bytes every excess verifier takes; and the joint walk b P + c Q of k_rp_expart_mulcheck alone, through its test hook.

The reference side is the host protocol code over the oracle backend (tests/rp_backends.py): rangeproof.excess_part_*_host restate the five calls over
the oracle's group law and hashlib, the oracle's inner_product the joint walk — never the library under test.  The pools are test_gpu_commit_open's 65
rows per setup; the job (19 sums over 70 parts) and its host reference are computed once per setup and shared."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import capi
from bulletproofspp_amd import rangeproof as RP
from rp_backends import OracleBackend
from test_gpu_commit_open import _case, _native, _no_point_x

pytestmark = pytest.mark.gpu

N, P = O.N, RP.FIELD_P
# one aux for every session of these jobs: the restatement has to be fed the same bytes.  A signer takes fresh randomness per session, as include/bppp.h
# demands (one aux under two sets of aggregates gives away the blinding)
AUX = hashlib.sha256(b"excess part aux").digest()
TAG = b"excess part tag"                                                                # the oracle tag of the tagged handle: Dm, Db and Dc hash it
SEED = hashlib.sha256(b"excess part seed").digest()
OK, MISMATCH, NOT_CANONICAL, BAD_R, NO_KEY, BAD_KEY, NONCE_INF, NO_AGG = 0, 1, 3, 4, 5, 6, 7, 8
NAMES = ["rec_test", "bin_test"]                                                        # a typed and a binary handle
SIZES = [1, 2, 3, 1, 2, 1, 2, 40, 1, 2, 3, 1, 2, 1, 2, 1, 2, 1, 2]                      # parts of the 19 sums: 70 in all
NONCE, KEY, PART, SIG = RP.EXCESS_PUBNONCE_BYTES, RP.EXCESS_KEY_BYTES, RP.EXCESS_PARTIAL_BYTES, RP.EXCESS_SIG_BYTES
_JOBS = {}


@pytest.fixture(scope="module")
def handles(gpu, oracle_lib):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _native(gpu, _case(oracle_lib, name)[0])
        return made[name]
    yield get
    for nat in made.values():
        nat.close()


@pytest.fixture
def flat_chunk():
    """bppp_test_rp_set_flat_chunk on one handle, restored afterwards"""
    tl, touched = capi.load_test_library(), []

    def set_(nat, items):
        if nat not in touched:
            touched.append(nat)
        assert tl.bppp_test_rp_set_flat_chunk(nat.h, items) == 0
    yield set_
    for nat in touched:
        assert tl.bppp_test_rp_set_flat_chunk(nat.h, 0) == 0


class _Dev:
    """arrays of one call in HBM, freed on exit; an int is an output buffer of that many bytes, filled with 0xA5"""

    def __init__(self, gpu, **arrays):
        self.gpu = gpu
        self.d = {k: gpu.to_device(np.full(v, 0xA5, dtype=np.uint8) if isinstance(v, int) else v) for k, v in arrays.items()}

    def __enter__(self):
        return self.d

    def __exit__(self, *exc):
        for p in self.d.values():
            self.gpu.free(p)


def _bytes(rows):
    return np.frombuffer(b"".join(rows) or b"\0", dtype=np.uint8)


def _rows(gpu, ptr, n, width):
    raw = gpu.download(ptr, (n * width,), np.uint8).tobytes()
    return [raw[t * width:(t + 1) * width] for t in range(n)]


def _neg(p):
    return None if p is None else (p[0], P - p[1])


def _flip(b33):
    return b33[:32] + bytes([b33[32] ^ 1])


def _plus_one(part):
    return RP._put((RP._get256(part) + 1) % N)


def _job(oracle_lib, name):
    """19 sums over 70 parts out of the pool: part i of sum t owns one commitment of the pool and signs with its blinding.  The host restatement of all
    five calls, once."""
    if name in _JOBS:
        return _JOBS[name]
    st, inputs, triples, pts, files = _case(oracle_lib, name)
    be, flat = OracleBackend(oracle_lib), [t for row in triples for t in row]
    rng = random.Random(101)
    owners = [[rng.randrange(len(flat)) for _ in range(sz)] for sz in SIZES]
    part_start = [0]
    for g in owners:
        part_start.append(part_start[-1] + len(g))
    entries = [RP.tally_entry(j, False) for g in owners for j in g]
    es = [flat[j][2] % N for g in owners for j in g]
    msgs = [hashlib.sha256(b"excess part msg %d" % t).digest() for t in range(len(SIZES))]
    part_msgs = [msgs[t] for t, g in enumerate(owners) for _ in g]
    _, _, B = RP._excess_bases(st)
    J = dict(st=st, files=files, flat=flat, part_start=part_start, entries=entries, es=es, msgs=msgs, part_msgs=part_msgs)
    J["keys"] = [RP.excess_key33(oracle_lib.mul(e, B)) for e in es]
    J["nonces"] = [RP.excess_part_nonces_host(be, st, e, m, AUX)[1] for e, m in zip(es, part_msgs)]
    groups = lambda rows: [rows[part_start[t]:part_start[t + 1]] for t in range(len(SIZES))]
    agg = [RP.excess_part_aggregate_host(be, st, pn, k) for pn, k in zip(groups(J["nonces"]), groups(J["keys"]))]
    assert [a[0] for a in agg] == [OK] * len(SIZES)
    J["agg_nonces"], J["agg_keys"] = [a[1] for a in agg], [a[2] for a in agg]
    part_agg = lambda rows: [rows[t] for t, g in enumerate(owners) for _ in g]
    signed = [RP.excess_part_sign_host(be, st, e, m, AUX, an, ak) for e, m, an, ak in zip(es, part_msgs, part_agg(J["agg_nonces"]), part_agg(J["agg_keys"]))]
    assert [s for s, _ in signed] == [OK] * len(es)
    J["partials"] = [p for _, p in signed]
    combined = [RP.excess_part_combine_host(be, st, pn, k, pt, m) for pn, k, pt, m in zip(groups(J["nonces"]), groups(J["keys"]), groups(J["partials"]), msgs)]
    assert [c[0] for c in combined] == [OK] * len(SIZES) and [c[2] for c in combined] == J["agg_keys"]
    J["sigs"] = [c[1] for c in combined]
    J["claims"] = RP.tally_claims_host(flat, part_start, entries)
    J["part_agg"], J["groups"] = part_agg, groups
    _JOBS[name] = J
    return J


# ----------------------------------------------------------------------------- 1. the joint walk alone against the oracle's inner product
def test_joint_walk_equals_oracle(gpu, oracle_lib, handles):
    st, _, _, pts, _ = _case(oracle_lib, "rec_test")
    nat, ec, tl = handles("rec_test"), oracle_lib, capi.load_test_library()
    rng = random.Random(7)
    g, H0, H1 = st.g, st.hs[0], st.hs[1]
    special = [0, 1, N - 1, 2**256 - 1, 2, 3, N, N + 1] + [2**k for k in (31, 32, 64, 129, 255)] + [2**k - 1 for k in (32, 33, 128, 255)]
    pairs = [(g, H0), (H0, H1), (H1, g), (g, g), (H0, H0), (H1, _neg(H1)), (_neg(g), g), (None, H0), (H1, None), (None, None), (pts[3][0], pts[4][0])]
    cases = [(b, p, c, q) for p, q in pairs for b, c in ((0, 0), (1, 1), (1, N - 1), (N - 1, 1), (2**256 - 1, 2**256 - 1), (0, 5), (5, 0), (2**255, 2**255 - 1), (2**128 - 1, 2**128))]
    cases += [(rng.choice(special), p, rng.randrange(2**256), q) for p, q in pairs for _ in range(2)]
    cases += [(rng.randrange(2**256), p, rng.choice(special), q) for p, q in pairs for _ in range(2)]
    cases += [(rng.randrange(2**256), p, rng.randrange(2**256), q) for p, q in pairs]
    cases += [(b, g, c, g) for b in special[:4] for c in special[:4]]                   # b + c = 0, 1, n mod n on one point
    rng.shuffle(cases)

    def want(b, p, c, q):
        terms = [(s % N, x) for s, x in ((b, p), (c, q)) if x is not None and s % N]
        return ec.inner_product(terms) if terms else None
    lo = 0
    for count in (1, 4, 16, 17, 65):                                                    # partial wavefronts, partial last blocks, more than one block
        part = cases[lo:lo + count]
        assert len(part) == count
        d = [gpu.to_device(capi.scalars_to_array([b for b, _, _, _ in part])), gpu.to_device(capi.points_to_array([p for _, p, _, _ in part])),
             gpu.to_device(capi.scalars_to_array([c for _, _, c, _ in part])), gpu.to_device(capi.points_to_array([q for _, _, _, q in part])), gpu.alloc(64 * count)]
        try:
            assert tl.bppp_test_rp_excess_mul2(nat.h, count, *d) == 0
            out = gpu.download(d[4], (count, 8), np.uint64)
        finally:
            for q in d:
                gpu.free(q)
        assert [capi.array_to_point(out[i]) for i in range(count)] == [want(*c) for c in part], count
        lo += count
    # the rest in one launch: every case is walked once
    part = cases[lo:]
    d = [gpu.to_device(capi.scalars_to_array([b for b, _, _, _ in part])), gpu.to_device(capi.points_to_array([p for _, p, _, _ in part])),
         gpu.to_device(capi.scalars_to_array([c for _, _, c, _ in part])), gpu.to_device(capi.points_to_array([q for _, _, _, q in part])), gpu.alloc(64 * len(part))]
    try:
        assert tl.bppp_test_rp_excess_mul2(nat.h, len(part), *d) == 0
        out = gpu.download(d[4], (len(part), 8), np.uint64)
    finally:
        for q in d:
            gpu.free(q)
    assert [capi.array_to_point(out[i]) for i in range(len(part))] == [want(*c) for c in part]


# ----------------------------------------------------------------------------- 2. end to end: every output is the host restatement's bytes
@pytest.mark.parametrize("name", NAMES)
def test_end_to_end(gpu, oracle_lib, handles, name):
    nat, J, typed = handles(name), _job(oracle_lib, name), name != "bin_test"
    ps, ns, npart = J["part_start"], len(SIZES), len(J["es"])
    assert nat.excess_keys(J["es"]) == J["keys"]
    assert nat.excess_part_nonces(J["es"], J["part_msgs"], AUX, want_status=True) == (J["nonces"], [OK] * npart)
    assert nat.excess_part_nonces(J["es"], J["part_msgs"], AUX) == J["nonces"]
    assert nat.excess_part_aggregate(ps, J["nonces"], J["keys"], want_status=True) == (J["agg_nonces"], J["agg_keys"], [OK] * ns)
    assert nat.excess_part_sign(J["es"], J["part_msgs"], AUX, J["part_agg"](J["agg_nonces"]), J["part_agg"](J["agg_keys"]), want_status=True) == (J["partials"], [OK] * npart)
    assert nat.excess_part_verify(ps, J["nonces"], J["keys"], J["partials"], J["msgs"]) == ([OK] * npart, [OK] * ns)
    assert nat.excess_part_combine(ps, J["nonces"], J["keys"], J["partials"], J["msgs"], want_status=True, want_keys=True) == (J["sigs"], [OK] * ns, J["agg_keys"])
    assert nat.excess_part_combine(ps, J["nonces"], J["keys"], J["partials"], J["msgs"]) == J["sigs"]
    # the 65 bytes under every verifier there is: the stated key, the pool with the public claim, and the sums against the aggregated key
    assert nat.excess_verify_keys_each(J["agg_keys"], J["msgs"], J["sigs"]) == [OK] * ns
    assert nat.excess_verify_keys_batch(J["agg_keys"], J["msgs"], J["sigs"], SEED, want_status=True)[:2] == (True, [OK] * ns)
    public = [(a, ty) if typed else (a,) for a, ty, _ in J["claims"]]
    assert nat.excess_verify_each(J["files"], ps, J["entries"], public, J["msgs"], J["sigs"]) == [OK] * ns
    sums_claims = [(a, ty, 0) if typed else (a, 0) for a, ty, _ in J["claims"]]
    assert nat.excess_sums_each(J["files"], ps, J["entries"], sums_claims, list(range(ns + 1)), J["agg_keys"]) == [OK] * ns
    # the _device variants: the same bytes in HBM
    psa = np.array(ps, dtype=np.uint32)
    with _Dev(gpu, bl=capi.scalars_to_array(J["es"]), pm=_bytes(J["part_msgs"]), m=_bytes(J["msgs"]), ps=psa, k=_bytes(J["keys"]), pn=npart * NONCE, an=ns * NONCE, ak=ns * KEY,
              pan=_bytes(J["part_agg"](J["agg_nonces"])), pak=_bytes(J["part_agg"](J["agg_keys"])), pt=npart * PART, sg=ns * SIG, ak2=ns * KEY) as d:
        assert nat.excess_part_nonces_device(npart, d["bl"], d["pm"], d["pn"], AUX, want_status=True) == [OK] * npart
        assert _rows(gpu, d["pn"], npart, NONCE) == J["nonces"]
        assert nat.excess_part_aggregate_device(ns, npart, d["ps"], d["pn"], d["k"], d["an"], d["ak"], want_status=True) == [OK] * ns
        assert _rows(gpu, d["an"], ns, NONCE) == J["agg_nonces"] and _rows(gpu, d["ak"], ns, KEY) == J["agg_keys"]
        assert nat.excess_part_sign_device(npart, d["bl"], d["pm"], d["pan"], d["pak"], d["pt"], AUX, want_status=True) == [OK] * npart
        assert _rows(gpu, d["pt"], npart, PART) == J["partials"]
        assert nat.excess_part_verify_device(ns, npart, d["ps"], d["pn"], d["k"], d["pt"], d["m"]) == ([OK] * npart, [OK] * ns)
        assert nat.excess_part_combine_device(ns, npart, d["ps"], d["pn"], d["k"], d["pt"], d["m"], d["sg"], d["ak2"], want_status=True) == [OK] * ns
        assert _rows(gpu, d["sg"], ns, SIG) == J["sigs"] and _rows(gpu, d["ak2"], ns, KEY) == J["agg_keys"]
        assert nat.excess_part_combine_device(ns, npart, d["ps"], d["pn"], d["k"], d["pt"], d["m"], d["sg"]) is None
    # one partial off by one in the long group and in a pair: the signatures fail and the check names those parts alone
    forged = list(J["partials"])
    culprits = (ps[7] + 23, ps[1] + 1)
    for p in culprits:
        forged[p] = _plus_one(forged[p])
    sigs = nat.excess_part_combine(ps, J["nonces"], J["keys"], forged, J["msgs"])
    assert nat.excess_verify_keys_each(J["agg_keys"], J["msgs"], sigs) == [MISMATCH if t in (7, 1) else OK for t in range(ns)]
    assert nat.excess_part_verify(ps, J["nonces"], J["keys"], forged, J["msgs"]) == ([MISMATCH if p in culprits else OK for p in range(npart)], [OK] * ns)
    assert nat.excess_part_nonces([], [], AUX) == [] and nat.excess_part_sign([], [], AUX, [], []) == []


# ----------------------------------------------------------------------------- 3. every verdict, in the header's order
@pytest.mark.parametrize("name", NAMES)
def test_signer_verdicts(gpu, oracle_lib, handles, name):
    """The signer's NONCE (a hash that is zero) and round 2's NONCE_INFINITY (R1agg = - b R2agg with b a hash over R1agg) need a preimage: no input
    reaches them."""
    nat, J, be = handles(name), _job(oracle_lib, name), OracleBackend(oracle_lib)
    st, bx = J["st"], RP._put(_no_point_x(oracle_lib))
    e, m, an, ak = J["es"][0], J["part_msgs"][0], J["agg_nonces"][0], J["agg_keys"][0]
    es = [e, 0, N, J["es"][1], 2**256 - 1]
    want = [RP.excess_part_nonces_host(be, st, x, m, AUX) for x in es]
    assert [s for s, _ in want] == [OK, RP.EXCESS_ZERO, RP.EXCESS_NOT_CANONICAL, OK, RP.EXCESS_NOT_CANONICAL] and want[1][1] == bytes(NONCE)
    assert nat.excess_part_nonces(es, [m] * 5, AUX, want_status=True) == ([p for _, p in want], [s for s, _ in want])
    with pytest.raises(capi.BpppError, match=r"rp_excess_part_nonces: part 1: .*zero"):
        nat.excess_part_nonces(es, [m] * 5, AUX)
    with pytest.raises(capi.BpppError, match=r"rp_excess_part_nonces: part 2: .*not canonical"):
        nat.excess_part_nonces([e, e, N, 0], [m] * 4, AUX)
    with _Dev(gpu, bl=capi.scalars_to_array(es), pm=_bytes([m] * 5), pn=5 * NONCE) as d:
        ax = np.frombuffer(AUX, dtype=np.uint8)
        assert gpu.lib.bppp_rp_excess_part_nonces_device(nat.h, 5, C.c_void_p(d["bl"]), C.c_void_p(d["pm"]), C.c_void_p(ax.ctypes.data), C.c_void_p(d["pn"]), None) == -1
        assert _rows(gpu, d["pn"], 5, NONCE) == [p for _, p in want]                   # the error stands and the rows are complete
    # round 2: the signer's own verdicts first, then the key, then the nonce points
    rows = [(e, an, ak), (0, an, ak[:32] + b"\x02"), (N, an[:32] + b"\x02" + an[33:], ak), (e, an, ak[:32] + b"\x02"), (e, an, bx + ak[32:]),
            (e, an[:33] + bx + an[65:], ak[:32] + b"\x02"), (e, an[:32] + b"\x02" + an[33:], ak), (e, an[:33] + bx + an[65:], ak)]
    want = [RP.excess_part_sign_host(be, st, x, m, AUX, a, k) for x, a, k in rows]
    assert [s for s, _ in want] == [OK, RP.EXCESS_ZERO, RP.EXCESS_NOT_CANONICAL, BAD_KEY, BAD_KEY, BAD_KEY, BAD_R, BAD_R] and want[0][1] == J["partials"][0]
    got = nat.excess_part_sign([x for x, _, _ in rows], [m] * len(rows), AUX, [a for _, a, _ in rows], [k for _, _, k in rows], want_status=True)
    assert got == ([p for _, p in want], [s for s, _ in want]) and got[0][3] == bytes(PART)
    with pytest.raises(capi.BpppError, match=r"rp_excess_part_sign: part 1: .*zero"):
        nat.excess_part_sign([x for x, _, _ in rows], [m] * len(rows), AUX, [a for _, a, _ in rows], [k for _, _, k in rows])
    assert gpu.lib.bppp_rp_excess_part_sign(nat.h, 1, None, None, None, None, None, None, None) == -1 and b"null input" in gpu.lib.bppp_last_error(gpu.h)
    # a size that cannot be: named as such, by the host variants too, which then upload nothing
    assert gpu.lib.bppp_rp_excess_part_sign(nat.h, 2**31, None, None, None, None, None, None, None) == -1 and b"n must be below 2^31" in gpu.lib.bppp_last_error(gpu.h)
    assert gpu.lib.bppp_rp_excess_part_nonces(nat.h, 2**31, None, None, None, None, None) == -1 and b"n must be below 2^31" in gpu.lib.bppp_last_error(gpu.h)


def _verdict_job(oracle_lib, J):
    """eight sums over the first parts of the shared job, one way to fail each: (part_start, nonces, keys, partials, msgs)"""
    bx = RP._put(_no_point_x(oracle_lib))
    n, k, p = J["nonces"], J["keys"], J["partials"]
    sums = [
        ([n[0]], [k[0]], [p[0]]),                                                       # 0: the first sum of the job as it is
        ([n[1], n[2]], [k[1], k[2][:32] + b"\x02"], [p[1], RP._put(N)]),                # 1: a key with sign byte 2 (and its s = n: the key is judged first)
        ([n[3], n[4], n[5]], [k[3], bx + k[4][32:], k[5]], [p[3], p[4], p[5]]),         # 2: a key's x without a point
        ([n[1][:33] + bx + n[1][65:], n[2]], [k[1], k[2]], [RP._put(N), p[2]]),         # 3: a nonce point without a point (and its s = n: s is judged first)
        ([n[1], n[2]], [k[1], _flip(k[1])], [p[1], p[2]]),                              # 4: X_2 = - X_1
        ([n[1], _flip(n[1][:33]) + n[2][33:]], [k[1], k[2]], [p[1], p[2]]),             # 5: R1_2 = - R1_1
        ([n[1], n[2]], [k[1], k[2]], [p[1], RP._put(N)]),                               # 6: s = n
        ([n[1], n[2]], [k[1], k[2]], [_plus_one(p[1]), p[2]]),                          # 7: the second sum of the job with one partial off by one
    ]
    part_start = [0]
    for s in sums:
        part_start.append(part_start[-1] + len(s[0]))
    flat = lambda i: [row for s in sums for row in s[i]]
    msgs = [J["msgs"][0]] + [J["msgs"][1]] * 7
    return part_start, flat(0), flat(1), flat(2), msgs


@pytest.mark.parametrize("name", NAMES)
def test_group_verdicts(gpu, oracle_lib, handles, name):
    nat, J, be = handles(name), _job(oracle_lib, name), OracleBackend(oracle_lib)
    st = J["st"]
    ps, nonces, keys, partials, msgs = _verdict_job(oracle_lib, J)
    ns, npart = len(ps) - 1, len(nonces)
    grp = lambda rows: [rows[ps[t]:ps[t + 1]] for t in range(ns)]
    agg = [RP.excess_part_aggregate_host(be, st, a, b) for a, b in zip(grp(nonces), grp(keys))]
    sum_want = [OK, BAD_KEY, BAD_KEY, BAD_R, NO_KEY, NONCE_INF, OK, OK]
    assert [a[0] for a in agg] == sum_want and agg[4][1:] == (bytes(NONCE), bytes(KEY))
    assert nat.excess_part_aggregate(ps, nonces, keys, want_status=True) == ([a[1] for a in agg], [a[2] for a in agg], sum_want)
    with pytest.raises(capi.BpppError, match=r"rp_excess_part_aggregate: sum 1: a key of the group"):
        nat.excess_part_aggregate(ps, nonces, keys)
    ver = [RP.excess_part_verify_host(be, st, a, b, c, m) for a, b, c, m in zip(grp(nonces), grp(keys), grp(partials), msgs)]
    # the part that does not lift reads BAD_KEY or BAD_R; its cosigners, whose own rows are sound, read NO_AGGREGATE (sum 3: its own s = n comes first)
    part_want = [OK, NO_AGG, BAD_KEY, NO_AGG, BAD_KEY, NO_AGG, NOT_CANONICAL, NO_AGG, NO_KEY, NO_KEY, NONCE_INF, NONCE_INF, OK, NOT_CANONICAL, MISMATCH, OK]
    assert [v for vs, _ in ver for v in vs] == part_want and [s for _, s in ver] == sum_want
    assert nat.excess_part_verify(ps, nonces, keys, partials, msgs) == (part_want, sum_want)
    com = [RP.excess_part_combine_host(be, st, a, b, c, m) for a, b, c, m in zip(grp(nonces), grp(keys), grp(partials), msgs)]
    assert [c[0] for c in com] == sum_want and com[0][1] == J["sigs"][0] and com[5][1:] == (bytes(SIG), bytes(KEY))
    assert nat.excess_part_combine(ps, nonces, keys, partials, msgs, want_status=True, want_keys=True) == ([c[1] for c in com], sum_want, [c[2] for c in com])
    with pytest.raises(capi.BpppError, match=r"rp_excess_part_combine: sum 1: a key of the group"):
        nat.excess_part_combine(ps, nonces, keys, partials, msgs)
    sigs = [c[1] for c in com]
    assert nat.excess_verify_keys_each([com[t][2] for t in (0, 6, 7)], [msgs[t] for t in (0, 6, 7)], [sigs[t] for t in (0, 6, 7)]) == [OK, MISMATCH, MISMATCH]
    # without a status array the refusal is the call's error, and the rows are as they would be with one
    with _Dev(gpu, ps=np.array(ps, dtype=np.uint32), pn=_bytes(nonces), k=_bytes(keys), pt=_bytes(partials), m=_bytes(msgs), an=ns * NONCE, ak=ns * KEY, sg=ns * SIG) as d:
        p = C.c_void_p
        assert gpu.lib.bppp_rp_excess_part_aggregate_device(nat.h, ns, npart, p(d["ps"]), p(d["pn"]), p(d["k"]), p(d["an"]), p(d["ak"]), None) == -1
        assert b"sum 1:" in gpu.lib.bppp_last_error(gpu.h)
        assert _rows(gpu, d["an"], ns, NONCE) == [a[1] for a in agg] and _rows(gpu, d["ak"], ns, KEY) == [a[2] for a in agg]
        assert gpu.lib.bppp_rp_excess_part_combine_device(nat.h, ns, npart, p(d["ps"]), p(d["pn"]), p(d["k"]), p(d["pt"]), p(d["m"]), p(d["sg"]), None, None) == -1
        assert b"sum 1:" in gpu.lib.bppp_last_error(gpu.h) and _rows(gpu, d["sg"], ns, SIG) == sigs


# ----------------------------------------------------------------------------- 4. argument errors: an error code, and no output is written
def test_group_errors(gpu, oracle_lib, handles):
    nat, J, lib = handles("rec_test"), _job(oracle_lib, "rec_test"), gpu.lib
    ps, ns, npart = J["part_start"], len(SIZES), len(J["es"])
    down = list(ps)
    down[5] = down[4] - 1
    short = ps[:-1] + [npart - 1]
    empty = list(ps)
    empty[3] = empty[2]
    vp = lambda a: C.c_void_p(a.ctypes.data)
    pn, k, pt, m = _bytes(J["nonces"]), _bytes(J["keys"]), _bytes(J["partials"]), _bytes(J["msgs"])
    for bad, text in ((down, r"part_start\[5\] = %d " % down[5]), (short, r"part_start\[%d\] = %d .*nparts = %d" % (ns, npart - 1, npart)), (empty, r"part_start: sum 2 has no part")):
        with pytest.raises(capi.BpppError, match=r"rp_excess_part_aggregate: " + text):
            nat.excess_part_aggregate(bad, J["nonces"], J["keys"])
        with pytest.raises(capi.BpppError, match=r"rp_excess_part_verify: " + text):
            nat.excess_part_verify(bad, J["nonces"], J["keys"], J["partials"], J["msgs"])
        with pytest.raises(capi.BpppError, match=r"rp_excess_part_combine: " + text):
            nat.excess_part_combine(bad, J["nonces"], J["keys"], J["partials"], J["msgs"])
        arr = np.array(bad, dtype=np.uint32)
        an, ak, sg = (np.full(ns * w, 0xA5, dtype=np.uint8) for w in (NONCE, KEY, SIG))
        status, pstatus = np.full(ns, 0xA5A5A5A5, dtype=np.uint32), np.full(npart, 0xA5A5A5A5, dtype=np.uint32)
        assert lib.bppp_rp_excess_part_aggregate(nat.h, ns, npart, vp(arr), vp(pn), vp(k), vp(an), vp(ak), vp(status)) == -1
        assert lib.bppp_rp_excess_part_verify(nat.h, ns, npart, vp(arr), vp(pn), vp(k), vp(pt), vp(m), vp(pstatus), vp(status)) == -1
        assert lib.bppp_rp_excess_part_combine(nat.h, ns, npart, vp(arr), vp(pn), vp(k), vp(pt), vp(m), vp(sg), vp(ak), vp(status)) == -1
        assert all((a == 0xA5).all() for a in (an, ak, sg)) and (status == 0xA5A5A5A5).all() and (pstatus == 0xA5A5A5A5).all()
    arr = np.array(ps, dtype=np.uint32)
    status = np.zeros(npart, dtype=np.uint32)
    assert lib.bppp_rp_excess_part_verify(nat.h, ns, npart, vp(arr), vp(pn), vp(k), vp(pt), vp(m), None, None) == -1 and b"null input" in lib.bppp_last_error(gpu.h)
    assert lib.bppp_rp_excess_part_verify(nat.h, ns, npart, vp(arr), vp(pn), vp(k), None, vp(m), vp(status), None) == -1 and b"null input" in lib.bppp_last_error(gpu.h)
    assert lib.bppp_rp_excess_part_aggregate(nat.h, ns, 2**31, vp(arr), vp(pn), vp(k), vp(pn), vp(k), None) == -1 and b"below 2^31" in lib.bppp_last_error(gpu.h)
    assert lib.bppp_rp_excess_part_verify(nat.h, ns, npart, vp(arr), vp(pn), vp(k), vp(pt), vp(m), vp(status), None) == 0 and list(status) == [OK] * npart
    assert lib.bppp_rp_excess_part_aggregate(nat.h, 0, 0, None, None, None, None, None, None) == 0


# ----------------------------------------------------------------------------- 5. several passes of whole sums give the bytes of one pass
@pytest.mark.parametrize("name", NAMES)
def test_passes(gpu, oracle_lib, handles, flat_chunk, name):
    nat, J, be = handles(name), _job(oracle_lib, name), OracleBackend(oracle_lib)
    ps, ns, npart = J["part_start"], len(SIZES), len(J["es"])
    forged = list(J["partials"])
    forged[ps[9] + 1] = _plus_one(forged[ps[9] + 1])
    want_verify = ([MISMATCH if p == ps[9] + 1 else OK for p in range(npart)], [OK] * ns)
    for items in (160, 164, 280):                                                       # 40, 41 and 70 parts a pass: the long group alone, with a neighbour, and one pass
        flat_chunk(nat, items)
        assert nat.excess_part_nonces(J["es"], J["part_msgs"], AUX) == J["nonces"]
        assert nat.excess_part_aggregate(ps, J["nonces"], J["keys"]) == (J["agg_nonces"], J["agg_keys"])
        assert nat.excess_part_sign(J["es"], J["part_msgs"], AUX, J["part_agg"](J["agg_nonces"]), J["part_agg"](J["agg_keys"])) == J["partials"]
        assert nat.excess_part_verify(ps, J["nonces"], J["keys"], forged, J["msgs"]) == want_verify
        assert nat.excess_part_combine(ps, J["nonces"], J["keys"], J["partials"], J["msgs"], want_keys=True) == (J["sigs"], None, J["agg_keys"])
    flat_chunk(nat, 64)                                                                 # 16 parts a pass: the group of 40 does not fit
    text = r"part_start: sum 7 has 40 parts, more than the 16 of one pass"
    with pytest.raises(capi.BpppError, match=r"rp_excess_part_aggregate: " + text):
        nat.excess_part_aggregate(ps, J["nonces"], J["keys"])
    with pytest.raises(capi.BpppError, match=r"rp_excess_part_verify: " + text):
        nat.excess_part_verify(ps, J["nonces"], J["keys"], J["partials"], J["msgs"])
    with pytest.raises(capi.BpppError, match=r"rp_excess_part_combine: " + text):
        nat.excess_part_combine(ps, J["nonces"], J["keys"], J["partials"], J["msgs"])
    assert nat.excess_part_sign(J["es"], J["part_msgs"], AUX, J["part_agg"](J["agg_nonces"]), J["part_agg"](J["agg_keys"])) == J["partials"]      # sessions have no groups


# ----------------------------------------------------------------------------- 6. a handle with an oracle tag: the three domains hash it
def test_tagged_handle(gpu, oracle_lib):
    st, _, triples, _, _ = _case(oracle_lib, "rec_test")
    be, flat = OracleBackend(oracle_lib), [t for row in triples for t in row]
    _, _, B = RP._excess_bases(st)
    es, msg = [flat[j][2] % N for j in (3, 11, 20)], hashlib.sha256(b"tagged").digest()
    keys = [RP.excess_key33(oracle_lib.mul(e, B)) for e in es]
    nonces = [RP.excess_part_nonces_host(be, st, e, msg, AUX, TAG)[1] for e in es]
    _, an, ak = RP.excess_part_aggregate_host(be, st, nonces, keys)
    partials = [RP.excess_part_sign_host(be, st, e, msg, AUX, an, ak, TAG)[1] for e in es]
    status, sig, _ = RP.excess_part_combine_host(be, st, nonces, keys, partials, msg, TAG)
    assert status == OK and RP.excess_verify_key_host(be, st, ak, msg, sig, TAG) == OK
    assert nonces != [RP.excess_part_nonces_host(be, st, e, msg, AUX)[1] for e in es]              # the tag reaches Dm
    nat = RP.NativeRangeProofs(gpu, st, oracle_tag=TAG)
    try:
        assert nat.excess_part_nonces(es, [msg] * 3, AUX) == nonces
        assert nat.excess_part_aggregate([0, 3], nonces, keys) == ([an], [ak])
        assert nat.excess_part_sign(es, [msg] * 3, AUX, [an] * 3, [ak] * 3) == partials             # Db in b, Dc in c
        assert nat.excess_part_verify([0, 3], nonces, keys, partials, [msg]) == ([OK] * 3, [OK])
        assert nat.excess_part_combine([0, 3], nonces, keys, partials, [msg]) == [sig]
        assert nat.excess_verify_keys_each([ak], [msg], [sig]) == [OK]
    finally:
        nat.close()
