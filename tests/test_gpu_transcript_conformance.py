"""The transcript layer under every challenge — decimal `show` of coordinates, the per-proof text builders, the two-wavefront SHA-256 over
header <> text suffix, and the prover's randomness — against a plain restatement: hashlib.sha256 over str(int).

Kernels under test: dec_convert / dec_write_backward and rp_hash_to_fr_pc / rp_msg_word (csrc/rphash.hip.h), k_rp_text, k_rp_text_lds, k_rp_hash,
k_rp_hash_bound (csrc/rp.hip), k_rpp_text_prepend, k_rpp_text_prepend_small, k_rpp_hash, k_rpp_hash_bound, k_rpp_draws (csrc/rpp_transcript.hip).
Every expected value is computed here:  decode_field (sha256 (tag [<> binding] <> str(n) <> str(npoints) <> concat (str(x) <> str(y))));  none
comes from the library, and none depends on a proof being valid (the verifier returns its challenges whatever the verdict).

 a. the corpus (CPU, unmarked): coordinates at every decimal length 1 .. 78, at every border of the nine 9-digit chunks, with zero middle chunks;
    x values ON the curve at every length (the verifier only shows what decodes) with both sign bits and aliases x + p; and, for every batch that
    is hashed on the device, message lengths at every residue mod 64, text pointers at every alignment mod 4, headers of 64 bytes and of lengths
    that are no multiple of 4 — by construction, checked before any GPU call;
 b. the verifier: crafted files of six setups (the four of the decode conformance test, one of 272 transcript points — two points per scan
    thread and the largest LDS launch of k_rp_text_lds — and one above the 272 / 273 threshold, which runs k_rp_text), batches of 64 + 37
    proofs, tags of length 0, 3 and the longest a header admits, device and host hashing, bound and unbound;
 c. the provers' transcript through bppp_test_rpp_transcript: 255 and 256 proofs (k_rpp_text_prepend / _small), calls of 1, 2, 8, 9 and 300 points;
 d. k_rpp_draws through bppp_test_rpp_draws at the counter and padding borders."""
import ctypes as C
import hashlib
import json
import os
import random

import numpy as np
import pytest

import pyoracle as O
from bulletproofspp_amd import encoding as E
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import TestRppCall, load_test_library
from rp_backends import OracleBackend
from test_gpu_decode_conformance import SETUPS, Layout, Lift
from test_rangeproof import EXAMPLES

P, N = E.P, RP.N
HDR_MAX, BINDING = 64, 32                                        # a header is at most 64 bytes; a bound header holds 32 binding bytes behind the tag
SYN_LDS, SYN_BIG = "synthetic 272", "synthetic 344"              # npts of the two synthetic setups
ALL_SETUPS = SETUPS + [SYN_LDS, SYN_BIG]
BATCH = 64 + 37                                                  # the last hash workgroup partly inactive; hash kinds share workgroups across their tails
TAG3 = b"tcf"


# ----------------------------------------------------------------------------- the restatement
def show(pt):
    return str(pt[0]).encode() + str(pt[1]).encode()


def challenge(tag, n, npoints, text):
    """shaOracle (app/Main.hs:75-80): tag already holds the binding of a bound call"""
    return RP.decode_field(hashlib.sha256(tag + str(n).encode() + str(npoints).encode() + text).digest(), N)


def chunk_class(v):
    """(index of the top 9-digit chunk, decimal digits of that chunk, whether a chunk below the top is zero) — what dec_convert branches on"""
    ch = [(v // 10**(9 * c)) % 10**9 for c in range(9)]
    top = max([c for c in range(9) if ch[c]] or [0])
    return top, len(str(ch[top])), any(ch[c] == 0 for c in range(top))


def text_lds_bytes(npts):
    """rp_text_lds_bytes (csrc/rp.hip): off[npts + 1] | len[2 npts] | chunks[2 npts][9] words, rounded to 16 bytes, then the text image"""
    stride = ((npts * 2 * 78 + 15) & ~15) + 16
    return ((npts + 1 + 2 * npts + 18 * npts) * 4 + 15) // 16 * 16 + stride


# ----------------------------------------------------------------------------- a. the corpus
def coord_corpus():
    rnd = random.Random("transcript conformance coordinates")
    cs = [0, 1, 7, 9, 10]
    for k in range(1, 78):
        cs += [10**k - 1, 10**k, 10**k + 1]
    cs += [10**27 + 5, 10**72 + 10**9, 10**45 + 10**18 + 3, 10**77 + 10**36]          # zero chunks below the top one
    cs += [P - 1, 2**255, 10**77 - 1, 10**77]                                          # 10^77 - 1: the largest 77-digit value; 10^77: the smallest of 78
    cs += [rnd.randrange(P) for _ in range(300)]
    return list(dict.fromkeys(cs))


def check_coord_corpus(cs):
    assert all(0 <= v < P for v in cs) and len(set(cs)) == len(cs)
    assert {len(str(v)) for v in cs} == set(range(1, 79))
    cls = [chunk_class(v) for v in cs]
    assert {t for t, _, _ in cls} == set(range(9))
    assert {(t, d) for t, d, _ in cls} >= {(t, d) for t in range(8) for d in range(1, 10)}       # every digit count of the top chunk, at every index
    assert {d for t, d, _ in cls if t == 8} == set(range(1, 7))                                  # ... the ninth chunk of a value below p has 1 .. 6 digits
    assert sum(z for _, _, z in cls) >= 8
    for k in (1, 2, 3, 4, 5, 6, 7, 8, 9):                         # the thresholds of ndigits9 themselves, as top chunk: 10^k - 1 | 10^k
        if k < 9:
            assert 10**k in cs
        assert 10**k - 1 in cs
    for special in (0, 1, 7, 9, 10, 10**27 + 5, 10**72 + 10**9, P - 1, 2**255, 10**77 - 1, 10**77):
        assert special in cs


_curve = {}


def curve_corpus(lift):
    """[(raw x as the file holds it, sign bit, (x, y) the text must show)]: for every decimal length two x on the curve, both signs, and aliases"""
    if "c" not in _curve:
        rnd = random.Random("transcript conformance curve")
        xs = []
        for L in range(1, 79):
            lo, hi = (0 if L == 1 else 10**(L - 1)), min(10**L, P)
            xs.append(next(x for x in range(lo, hi) if lift(x) is not None))               # the smallest x of L digits on the curve
            while True:
                x = rnd.randrange(lo, hi)
                if lift(x) is not None and x not in xs:
                    break
            xs.append(x)
        out = []
        for x in xs:
            for raw in [x] + ([x + P] if x + P < 2**256 else []):
                for sg in (0, 1):
                    y = lift(x)[1]
                    if (y > P - y) != bool(sg):
                        y = P - y
                    out.append((raw, sg, (x, y)))
        _curve["c"] = out
    return _curve["c"]


def check_curve_corpus(cc):
    assert {len(str(pt[0])) for _, _, pt in cc} == set(range(1, 79))
    for raw, sg, (x, y) in cc:
        assert raw % P == x and (y * y - x**3 - 7) % P == 0 and (y > P - y) == bool(sg)
    by_x = {}
    for raw, sg, _ in cc:
        by_x.setdefault(raw, set()).add(sg)
    assert all(s == {0, 1} for s in by_x.values())
    assert sum(raw >= P for raw, _, _ in cc) >= 6
    assert {chunk_class(pt[0])[0] for _, _, pt in cc} == set(range(9))
    assert {chunk_class(pt[0])[1] for _, _, pt in cc} == set(range(1, 10))


# ----------------------------------------------------------------------------- the setups (host side: no GPU)
_setups = {}


def host_setup(ec, name):
    """(setup, binary, Layout) of one of ALL_SETUPS; the layout from the setup alone, as bppp_rp_info reports it"""
    if name not in _setups:
        if name in SETUPS:
            schema = json.load(open(os.path.join(EXAMPLES, name, "schema.json")))
            binary = bool(schema.get("binary", False))
            st = (BRP if binary else RP).setup_from_schema(OracleBackend(ec), schema)
        else:
            # many one-digit ranges, like _setup of test_gpu_native_verify.py: npts = 2 rounds + 4 + ranges
            npts = int(name.split()[1])
            nr = next(r for r in range(1, npts) if 2 * RP.optimal_witness_size(r, 6, "NL")[0] + 4 + r == npts)
            rds = [RP.make_range_data(2, 0, 2, False, True, False) for _ in range(nr)]
            st, binary = RP.setup(OracleBackend(ec), O.hash_points(b"transcript conformance", 2 + 6 + nr), False, [], rds, "NL"), False
        nrp, nr, k, (fn, fl) = (2 if binary else 4), len(st.rds), st.rounds, st.final_lens
        npp = nrp + 2 * k
        shape = {"nranges": nr, "rounds": k, "final_norm": fn, "final_lin": fl, "coms_bytes": (nr + 7) // 8 + 32 * nr,
                 "proof_bytes": 32 * (fn + fl) + (npp + 7) // 8 + 32 * npp}
        _setups[name] = (st, binary, Layout(shape, nrp))
    return _setups[name]


def verifier_plan(L, binary):
    """(n, first text point) of every challenge in the order verify_batch returns them: the range-proof layer's, then the rounds' (last round
    first).  The text of a proof: its 2k response points in file order, the range-proof commitments, the input commitments; a challenge hashes
    the suffix from its first point (TypedReciprocal.hs:459-462, Binary.hs:209-213, Bulletproof.hs:374)."""
    k = L.k
    if binary:
        lead = [(n, 2 * k + 1) for n in (1, 2, 3)] + [(1, 2 * k)]
    else:
        lead = [(n, 2 * k + 2) for n in (1, 2, 3)] + [(n, 2 * k + 1) for n in (1, 2, 3)] + [(1, 2 * k)]
    return lead, [(1, 2 * i) for i in range(k)]


def tag_configs(L):
    """(tag, bound) of the device-hashed verifier batches: tags of 0 and 3 bytes and the longest the header rule tag <> str(n) <> str(count) admits"""
    digits = len(str(L.npts))                                     # the last round hashes all npts points: the longest count
    tag_u, tag_b = b"U" * (HDR_MAX - 1 - digits), b"B" * (HDR_MAX - BINDING - 1 - digits)
    return [(b"", False), (b"", True), (TAG3, False), (TAG3, True), (tag_u, False), (tag_b, True)]


_batches = {}


def verifier_batch(L, cc, name):
    """BATCH proofs as text-order lists of corpus entries.  Proof b: every position from the corpus in turn (so every entry is used), then the
    second point chosen so that the text pointer of the hashes that start at point 2 sits at alignment b mod 4, and the last two points so that the
    whole text has length b mod 64 — the challenge of the last round hashes all of it, so its message length takes every residue mod 64
    whatever the header."""
    if name not in _batches:
        rnd = random.Random("verifier batch " + name)
        order = list(cc)
        rnd.shuffle(order)
        tlen = lambda e: len(show(e[2]))
        by4, by64 = {}, {}
        for e in order:
            by4.setdefault(tlen(e) % 4, []).append(e)
            by64.setdefault(tlen(e) % 64, []).append(e)
        assert set(by4) == set(range(4))
        proofs, at = [], 0
        for b in range(BATCH):
            T = [order[(at + i) % len(order)] for i in range(L.npts)]
            at += L.npts
            T[1] = rnd.choice(by4[(b - tlen(T[0])) % 4])
            need = (b - sum(tlen(e) for e in T[:-2])) % 64        # ... by the last two points: one point's lengths do not reach every residue
            T[-2] = next(e for e in rnd.sample(order, len(order)) if (need - tlen(e)) % 64 in by64)
            T[-1] = rnd.choice(by64[(need - tlen(T[-2])) % 64])
            proofs.append(T)
        _batches[name] = proofs
    return _batches[name]


def verifier_messages(L, binary, proofs, tag, bound):
    """(header length, text-pointer alignment mod 4, message length) of every hash of the batch"""
    lead, es = verifier_plan(L, binary)
    out = []
    for T in proofs:
        lens = [len(show(e[2])) for e in T]
        for n, start in lead + es:
            hlen = len(tag) + (BINDING if bound else 0) + len(str(n)) + len(str(L.npts - start))
            out.append((hlen, sum(lens[:start]) % 4, hlen + sum(lens[start:])))
    return out


def check_messages(msgs, want_hdr64):
    assert {m % 64 for _, _, m in msgs} == set(range(64))         # 0: the padding block follows the last interior block; 55 | 56: the length fits | does not
    assert {a for _, a, _ in msgs} == {0, 1, 2, 3}
    assert all(h <= HDR_MAX for h, _, _ in msgs) and (HDR_MAX in {h for h, _, _ in msgs}) == want_hdr64
    return {h % 4 for h, _, _ in msgs}


def files_of(L, T, rnd):
    """text order -> file order: the range-proof commitments, the responses, then the inputs"""
    k2 = 2 * L.k
    pts = [(raw, sg) for raw, sg, _ in T[k2:k2 + L.nrp] + T[:k2] + T[k2 + L.nrp:]]
    return L.build([rnd.randrange(N) for _ in range(L.ns)], pts)


# the provers' transcript: oracle calls (points, count, first slot) of the two plans; 300 + 1 + 2 + 8 + 9 points fit the big synthetic setup
PLAN_A = [(300, 3, 0), (1, 1, 6), (2, 3, 3), (8, 1, 7), (9, 3, 4)]
PLAN_B = [(1, 3, 0), (9, 1, 7), (8, 3, 4), (2, 1, 6)]            # a transcript that STARTS with one point: (7, 5) in proof 0
_prover = {}


def prover_batch(B, plan, label):
    """points[c][b] = the (x, y) of call c of proof b: coordinates from the whole corpus in turn — text, not curve points"""
    key = (B, label)
    if key not in _prover:
        rnd = random.Random("prover batch %d %s" % key)
        cs = coord_corpus()
        rnd.shuffle(cs)
        at, pts = 0, []
        for m, _, _ in plan:
            per_call = []
            for b in range(B):
                per_call.append([(cs[(at + 2 * i) % len(cs)], cs[(at + 2 * i + 1) % len(cs)]) for i in range(m)])
                at += 2 * m + 1                                   # odd: every value turns up as x and as y
            pts.append(per_call)
        if label == "B":
            pts[0][0] = [(7, 5)]
        _prover[key] = pts
    return _prover[key]


def prover_expected(tag, plan, pts, b, binding=b""):
    """[challenges of call c] of proof b, and (header length, alignment, message length) of each hash: the text grows at its FRONT and ends 16
    bytes before a multiple of 16, so its start sits at -length mod 4"""
    text, total, out, msgs = b"", 0, [], []
    for (m, count, _), per_call in zip(plan, pts):
        text = b"".join(show(p) for p in per_call[b]) + text
        total += m
        out.append([challenge(tag + binding, n, total, text) for n in range(1, count + 1)])
        msgs += [(len(tag + binding) + len(str(n)) + len(str(total)), -len(text) % 4, len(tag + binding) + len(str(n)) + len(str(total)) + len(text))
                 for n in range(1, count + 1)]
    return out, msgs


def test_corpus_and_coverage(oracle_lib):
    """(a): everything a batch must contain, asserted on the CPU"""
    check_coord_corpus(coord_corpus())
    lift = Lift(oracle_lib)
    cc = curve_corpus(lift)
    check_curve_corpus(cc)
    # the threshold between the text kernels, from the formula: 272 points are the largest LDS launch, 273 take k_rp_text
    assert text_lds_bytes(272) == 65312 <= 64 * 1024 < text_lds_bytes(273) == 65552
    for name in ALL_SETUPS:
        st, binary, L = host_setup(oracle_lib, name)
        proofs = verifier_batch(L, cc, name)
        assert len(proofs) % 64 == 37
        used = {e for T in proofs for e in T}
        assert {len(str(e[2][0])) for e in used} == set(range(1, 79)) and any(e[0] >= P for e in used)
        hdr_mod4 = set()
        for tag, bound in tag_configs(L):
            longest = len(tag) + (BINDING if bound else 0) + 1 + len(str(L.npts)) == HDR_MAX
            assert longest == (tag not in (b"", TAG3))
            hdr_mod4 |= check_messages(verifier_messages(L, binary, proofs, tag, bound), longest)
        assert hdr_mod4 & {1, 2, 3}                               # headers that end inside a word
    assert host_setup(oracle_lib, SYN_LDS)[2].npts == 272 and (272 + 255) // 256 == 2        # two points per scan thread, through LDS
    big = host_setup(oracle_lib, SYN_BIG)[2].npts
    assert big >= 273 and big >= sum(m for m, _, _ in PLAN_A) and sum(m for m, _, _ in PLAN_A) > 256     # k_rp_text; the plan fits; per = 2 at m = 300
    for name in (SYN_LDS, SYN_BIG):                               # nothing of the synthetic setups is left out of a comparison: every point decodes
        assert all(lift(e[2][0]) is not None for T in verifier_batch(host_setup(oracle_lib, name)[2], cc, name) for e in T)
    # the provers' batches: the call sizes on both sides of the m <= 8 switch and of one point per scan thread, the borders of the padding
    for plan, label in ((PLAN_A, "A"), (PLAN_B, "B")):
        assert {m for m, _, _ in PLAN_A + PLAN_B} == {1, 2, 8, 9, 300} and {c for _, c, _ in plan} == {1, 3}
        for B in (255, 256):
            pts = prover_batch(B, plan, label)
            msgs = [m for b in range(B) for m in prover_expected(TAG3, plan, pts, b)[1]]
            assert {m % 64 for _, _, m in msgs} == set(range(64)) and {a for _, a, _ in msgs} == {0, 1, 2, 3} and {h % 4 for h, _, _ in msgs} & {1, 2, 3}
            seen = {v for per_call in pts for row in per_call for p in row for v in p}
            assert seen >= set(coord_corpus())                    # every corpus value goes through dec_convert


# ----------------------------------------------------------------------------- b. the verifier
@pytest.fixture(scope="module")
def lift(oracle_lib):
    return Lift(oracle_lib)


def _native(gpu, st, binary, tag):
    return (BRP.NativeBinaryRangeProofs if binary else RP.NativeRangeProofs)(gpu, st, oracle_tag=tag)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_SETUPS)
def test_verifier_challenges_of_crafted_files(gpu, oracle_lib, lift, name):
    st, binary, L = host_setup(oracle_lib, name)
    cc = curve_corpus(lift)
    proofs = verifier_batch(L, cc, name)
    rnd = random.Random("verifier files " + name)
    files = [files_of(L, T, rnd) for T in proofs]
    coms, prfs = [c for c, _ in files], [p for _, p in files]
    bindings = [hashlib.sha256(b"binding %d" % b).digest() for b in range(BATCH)]
    lead, es = verifier_plan(L, binary)
    texts = [[show(e[2]) for e in T] for T in proofs]
    suffix = [{start: b"".join(tx[start:]) for start in {s for _, s in lead + es}} for tx in texts]

    def expected(tag, bound):
        one = lambda b, plan: [challenge(tag + (bindings[b] if bound else b""), n, L.npts - s, suffix[b][s]) for n, s in plan]
        return [(one(b, lead), one(b, es)) for b in range(BATCH)]

    tl = load_test_library()
    want_kernel = 1 if text_lds_bytes(L.npts) <= 64 * 1024 else 0
    assert want_kernel == (0 if name == SYN_BIG else 1)
    seed = bytes(range(32))
    by_tag = {}
    for tag, bound in tag_configs(L):
        by_tag.setdefault(tag, []).append(bound)
    for tag, bounds in by_tag.items():
        nat = _native(gpu, st, binary, tag)
        try:
            assert Layout(nat.shape, L.nrp).npts == L.npts and nat.shape["challenges_per_proof"] == len(lead) + len(es)
            # the hashing routes: 0 = on the device; a value that covers the batch = the device's text, SHA-256 on the host cores
            routes = [(0, bound) for bound in bounds] + ([(BATCH, False)] if False in bounds and tag != TAG3 else [])
            for host_oracle_max, bound in routes:
                nat.set_option("host_oracle_max", host_oracle_max)
                _, _, chs = nat.verify_batch(coms, prfs, seed, want_challenges=True, bindings=bindings if bound else None)
                ran = C.c_int(-2)
                gpu._check(tl.bppp_test_rp_last_text_kernel(nat.h, C.byref(ran)), "bppp_test_rp_last_text_kernel")
                assert ran.value == want_kernel, (name, tag, ran.value)
                want = expected(tag, bound)
                for b in range(BATCH):
                    assert (list(chs[b][0]), list(chs[b][1])) == want[b], (name, len(tag), bound, host_oracle_max, b)
        finally:
            nat.close()


# ----------------------------------------------------------------------------- c. the provers' transcript
def _points_words(rows):
    return np.frombuffer(b"".join(x.to_bytes(32, "little") + y.to_bytes(32, "little") for row in rows for x, y in row), dtype=np.uint64).copy()


@pytest.fixture(scope="module")
def big_handle(gpu, oracle_lib):
    st, binary, _ = host_setup(oracle_lib, SYN_BIG)
    nat = _native(gpu, st, binary, TAG3)
    yield nat
    nat.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [255, 256])                         # m <= 8 && B >= 256: k_rpp_text_prepend_small, else k_rpp_text_prepend
@pytest.mark.parametrize("label", ["A", "B, bound"])
def test_prover_transcript(gpu, big_handle, B, label):
    plan, key, bound = (PLAN_A, "A", False) if label == "A" else (PLAN_B, "B", True)
    pts = prover_batch(B, plan, key)
    tl = load_test_library()
    calls = (TestRppCall * len(plan))(*[TestRppCall(m, c, s) for m, c, s in plan])
    words = np.concatenate([_points_words(per_call) for per_call in pts])
    bindings = [hashlib.sha256(b"prover binding %d" % b).digest() for b in range(B)]
    out = np.full((len(plan), B, 3, 4), 0xDEAD, dtype=np.uint64)
    gpu._check(tl.bppp_test_rpp_transcript(big_handle.h, B, C.cast(calls, C.c_void_p), len(plan), C.c_void_p(words.ctypes.data),
                                           C.c_char_p(b"".join(bindings)) if bound else None, C.c_void_p(out.ctypes.data)), "bppp_test_rpp_transcript")
    for b in range(B):
        want, _ = prover_expected(TAG3, plan, pts, b, bindings[b] if bound else b"")
        for c, (_, count, _) in enumerate(plan):
            got = [int.from_bytes(out[c, b, n].tobytes(), "little") for n in range(3)]
            assert got == want[c] + [0] * (3 - count), (label, B, b, c)


# ----------------------------------------------------------------------------- d. the provers' randomness
# prefix lengths: with 1 .. 4 counter digits, 0 .. 100 put prefix + digits on 55 | 56 and on 64; 51, 52 and 59 .. 62 add 63 and reach each of the four
# borders with every number of counter digits
DRAW_PREFIX_LENS = [0, 1, 45, 46, 47, 53, 54, 55, 63, 64, 100] + [51, 52, 59, 60, 61, 62]
DRAWS, DRAW_BATCH = 1001, 3                                       # counters 9 -> 10, 99 -> 100, 999 -> 1000; 3003 lanes: the last workgroup is partial


def test_draw_borders_are_reached():
    for d in (1, 2, 3, 4):                                        # message lengths 55 | 56 (the length fits the block | does not) and 63 | 64
        assert {55 - d, 56 - d, 63 - d, 64 - d} <= set(DRAW_PREFIX_LENS)
    assert (DRAWS * DRAW_BATCH) % 64 and DRAWS > 1000 and len(set(DRAW_PREFIX_LENS)) == len(DRAW_PREFIX_LENS)


@pytest.mark.gpu
@pytest.mark.parametrize("plen", DRAW_PREFIX_LENS)
def test_draws(gpu, plen):
    tl = load_test_library()
    rnd = random.Random("draws %d" % plen)
    prefixes = [bytes(rnd.randrange(256) for _ in range(plen)) for _ in range(DRAW_BATCH)]
    out = np.full((DRAW_BATCH, DRAWS, 4), 0xDEAD, dtype=np.uint64)
    gpu._check(tl.bppp_test_rpp_draws(gpu.h, b"".join(prefixes) if plen else None, plen, DRAW_BATCH, DRAWS, C.c_void_p(out.ctypes.data)), "bppp_test_rpp_draws")
    for b, pre in enumerate(prefixes):
        draw = RP.hash_to_scalar(pre)
        got = [int.from_bytes(out[b, c].tobytes(), "little") for c in range(DRAWS)]
        assert got == [draw(c) for c in range(DRAWS)], (plen, b)
