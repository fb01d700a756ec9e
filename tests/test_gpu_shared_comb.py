"""One comb table for the prover handles of a basis family (bppp_rp_share_comb, bppp_rp_comb_info) and the prover of a job of several
setups (bppp_rp_prove_mixed).  Every reference example is a setup over the one point stream "test points", so the table of a longer
basis contains the table of every shorter one: a handle that borrows it must write, byte for byte, the files it writes over a table of
its own, on every prover route; the table is allocated once and lives until its last user is gone.

Tables are forced with COMB_MIN = 1 and kept small with COMB_BITS = 6 (8 where the test measures memory): megabytes, not gigabytes."""
import hashlib
import json
import os
import random

import pytest

import pyoracle as O
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP
from bulletproofspp_amd.capi import BpppError
from test_rangeproof import EXAMPLES

pytestmark = pytest.mark.gpu

SEED = hashlib.sha256(b"shared comb seed").digest()
BITS = 6
MIB = 1 << 20
# free-memory checks: the runtime hands out device memory in 2 MiB granules and keeps small pools of its own, and a handle's first proof
# allocates workspaces; nothing here but the table is larger than a few MiB, so 64 MiB of slack separates "one table" (331 MiB at 8
# bits over the 1284 points of 128by64) from "two" or "none" with a wide margin
SLACK = 64 * MIB

_SETUPS = {}


def _schema(name):
    return json.load(open(os.path.join(EXAMPLES, name, "schema.json")))


def _setup(gpu, name, basis_seed=None):
    """the host setup of an example (cached: deriving the points is the slow part), optionally over another point stream"""
    key = (name, basis_seed)
    if key not in _SETUPS:
        schema = _schema(name)
        if basis_seed is not None:
            schema["basisSeed"] = basis_seed
        mod = BRP if schema.get("binary", False) else RP
        _SETUPS[key] = mod.setup_from_schema(RP.GpuBackend(gpu), schema)
    return _SETUPS[key]


def _handle(gpu, name, basis_seed=None, bits=BITS, **options):
    st = _setup(gpu, name, basis_seed)
    nat = (BRP.NativeBinaryRangeProofs if isinstance(st, BRP.SetupBRP) else RP.NativeRangeProofs)(gpu, st)
    nat.set_option("comb_min", 1)
    nat.set_option("comb_bits", bits)
    for k, v in options.items():
        nat.set_option(k, v)
    return nat


def _inputs(name, n, tag=b""):
    """n witnesses of an example: the shipped amounts with fresh blindings per proof"""
    wit = json.load(open(os.path.join(EXAMPLES, name, "witness.json")))
    binary = bool(_schema(name).get("binary", False))
    out = []
    for j in range(n):
        rows = RP.inputs_from_witness(wit, b"shared %s %s %d" % (tag, name.encode(), j))
        out.append([(v, bl) for v, _, bl in rows] if binary else rows)
    return out


def _prefixes(n, tag=b""):
    return [b"shared comb rnd %s %04d" % (tag, j) for j in range(n)]


def _basis_len(nat):
    return 1 + nat.shape["lin_len"] + nat.shape["norm_len"]


def _free():
    """free HBM of device 0 in bytes: hipMemGetInfo (what torch.cuda.mem_get_info reports) of the HIP runtime the library already runs
    on — a second runtime brought into the process by torch after the library's does not find the GPU"""
    import ctypes as C
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipSetDevice(0) == 0 and hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


# ----------------------------------------------------------------------------- 1. bytes: a borrowed table against an own one, every route
# (short, long): typed under typed, inner-product flavour under norm-linear, binary under typed, typed under binary
PAIRS = [("32by64", "128by64"), ("64bit", "128by64"), ("bin_test", "128by64"), ("64bit", "bin_test")]
# the prover routes the options select; both handles of a comparison get the same ones
ROUTES = {
    "stream": {},                                  # table in place: the whole proof one stream of kernels
    "fold_points": {"fold_points": 1},             # the point-folding argument although a table exists
    "host_algebra": {"host_algebra": 1},           # field algebra and hashing on the host
    "rebased": {},                                 # the fixed-basis argument re-based at level 2 (BPPP_NLB_REBASE, read when the argument starts)
    "split": {"split_min": 2},                     # two half-batches in flight, the second on the twin handle
}
NPROOFS = 5


@pytest.fixture(scope="module")
def donors(gpu):
    """the long handles, each with its table built once"""
    hs = {}
    for name in sorted({long for _, long in PAIRS}):
        hs[name] = _handle(gpu, name)
        hs[name].share_comb(hs[name])              # rp == donor: only forces the build
        assert hs[name].comb_info()["points"] == _basis_len(hs[name])
    yield hs
    for h in hs.values():
        h.close()


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("short,long", PAIRS)
def test_borrowed_table_gives_the_same_bytes(gpu, donors, monkeypatch, short, long, route):
    if route == "rebased":
        monkeypatch.setenv("BPPP_NLB_REBASE", "2")
    if route == "split":
        monkeypatch.setenv("BPPP_RP_SPLIT_MIN_BINARY", "2")     # a binary handle takes its split threshold when it is created
    own, borrower = _handle(gpu, short, **ROUTES[route]), _handle(gpu, short, **ROUTES[route])
    try:
        donor = donors[long]
        users = donor.comb_info()["users"]
        borrower.share_comb(donor)
        info = borrower.comb_info()
        assert info == donor.comb_info() and info["users"] == users + 1 and info["points"] == _basis_len(donor) > _basis_len(borrower)
        inputs, prefixes = _inputs(short, NPROOFS), _prefixes(NPROOFS)
        want = own.prove_batch(inputs, prefixes)
        got = borrower.prove_batch(inputs, prefixes)
        assert got == want
        assert borrower.comb_info() == info          # proving did not swap the table for an own one
        if route != "host_algebra":                  # (the host-algebra route builds no table of its own)
            assert own.comb_info()["points"] == _basis_len(own) and own.comb_info()["users"] == 1
        assert borrower.verify_batch([c for c, _ in got], [p for _, p in got], SEED)
    finally:
        own.close(); borrower.close()
    assert donors[long].comb_info()["users"] == users


# ----------------------------------------------------------------------------- 2. one table, not two
@pytest.fixture
def own_ctx():
    import bulletproofspp_amd as b
    ctx = b.Bppp(0)
    yield ctx
    ctx.close()


def test_sharing_allocates_one_table(own_ctx):
    long, short = _handle(own_ctx, "128by64", bits=8), _handle(own_ctx, "32by64", bits=8)
    try:
        assert long.comb_info() == short.comb_info() == {"window_bits": 0, "bytes": 0, "points": 0, "users": 0}
        before = _free()
        short.share_comb(long)                       # the donor has no table yet: built now
        drop = before - _free()
        a, b = long.comb_info(), short.comb_info()
        assert a == b and a["users"] == 2 and a["window_bits"] == 8 and a["points"] == _basis_len(long)
        assert a["bytes"] == 33 * a["points"] * 128 * 64          # ceil(257 / 8) windows x points x 2^7 multiples x 64 B
        print("table %d MiB, free HBM dropped by %d MiB" % (a["bytes"] // MIB, drop // MIB))
        assert a["bytes"] - SLACK <= drop <= a["bytes"] + SLACK    # about one table (331 MiB), not two
        short.share_comb(long)                       # again: nothing changes
        assert short.comb_info() == a and abs(before - _free() - drop) <= SLACK
    finally:
        long.close(); short.close()


# ----------------------------------------------------------------------------- 3. lifetime
@pytest.mark.parametrize("first", ["donor", "borrower"])
def test_table_lives_until_its_last_user(first):
    import bulletproofspp_amd as b
    before = _free()
    ctx = b.Bppp(0)                                  # a context of its own: its grow-only workspaces go with it
    long, short = _handle(ctx, "128by64", bits=8), _handle(ctx, "32by64", bits=8)
    try:
        short.share_comb(long)
        table = long.comb_info()["bytes"]
        keep, gone = (short, long) if first == "donor" else (long, short)
        name = "32by64" if keep is short else "128by64"
        inputs, prefixes = _inputs(name, 2), _prefixes(2)
        want = keep.prove_batch(inputs, prefixes)
        gone.close()
        info = keep.comb_info()
        assert info["users"] == 1 and info["bytes"] == table and info["points"] == _basis_len(long)
        assert before - _free() >= table - SLACK     # the table is still there
        assert keep.prove_batch(inputs, prefixes) == want
    finally:
        long.close(); short.close(); ctx.close()
    print("free HBM before %d MiB, after %d MiB" % (before // MIB, _free() // MIB))
    assert before - _free() <= SLACK                 # the last user took the table with it


def test_context_destroyed_before_its_handles():
    """include/bppp.h: a child handle keeps its context alive; the shared table goes with the last handle, in any order"""
    import bulletproofspp_amd as b
    before = _free()
    ctx = b.Bppp(0)
    long, short = _handle(ctx, "128by64", bits=8), _handle(ctx, "32by64", bits=8)
    short.share_comb(long)
    assert short.comb_info()["users"] == 2
    ctx.lib.bppp_ctx_destroy(ctx.h)                  # the context first ...
    ctx.h = None
    long.close()                                     # ... then the donor, then the borrower
    short.close()
    assert before - _free() <= SLACK


# ----------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_both_handles_usable(gpu):
    import bulletproofspp_amd as b
    short, long, other = _handle(gpu, "32bit"), _handle(gpu, "64bit"), _handle(gpu, "64bit", basis_seed="some other points")
    ctx2 = b.Bppp(0)
    far = _handle(ctx2, "64bit")
    try:
        assert _basis_len(long) > _basis_len(short) or pytest.fail("the pair is the wrong way round")
        for rp, donor, word in [(short, other, "extend"), (long, short, "extend"), (short, far, "contexts")]:
            with pytest.raises(BpppError) as e:
                rp.share_comb(donor)
            assert "(-1)" in str(e.value) and word in str(e.value), str(e.value)
            assert rp.comb_info()["users"] == 0 and donor.comb_info()["users"] == 0
        for name, h in [("32bit", short), ("64bit", long), ("64bit", other), ("64bit", far)]:
            files = h.prove_batch(_inputs(name, 2), _prefixes(2))
            assert h.verify_batch([c for c, _ in files], [p for _, p in files], SEED)
            assert h.comb_info()["users"] == 1
    finally:
        for h in (short, long, other, far):
            h.close()
        ctx2.close()


# ----------------------------------------------------------------------------- 5. nothing shares unless asked
def test_default_is_one_table_per_handle(gpu):
    a, b_ = _handle(gpu, "32bit"), _handle(gpu, "64bit")
    try:
        for name, h in (("32bit", a), ("64bit", b_)):
            h.prove_batch(_inputs(name, 2), _prefixes(2))
            info = h.comb_info()
            assert info["users"] == 1 and info["points"] == _basis_len(h) and info["window_bits"] == BITS
    finally:
        a.close(); b_.close()


# ----------------------------------------------------------------------------- 6. prove_mixed
# five setups of the one stream (typed, inner-product flavour, typed with types, binary), group sizes from 1 to 300, an empty group, and one
# setup over an unrelated stream
JOB = [("32bit", None, 300), ("64bit", None, 1), ("rec_test", None, 17), ("64by64", None, 0), ("32by64", None, 40), ("bin_test", None, 120),
       ("32bit", "some other points", 5)]


def _binary_net_inputs(nets, seed):
    """bin_test's shape with a net public amount per proof: one output in [3, 2^64), two assumed inputs; net + in1 + in2 - out = 0"""
    rnd = random.Random(seed)
    out = []
    for net in nets:
        i1, i2 = rnd.randrange(30, 2**40), rnd.randrange(30, 2**40)
        out.append([(net + i1 + i2, rnd.randrange(O.N)), (i1, rnd.randrange(O.N)), (i2, rnd.randrange(O.N))])
    return out


@pytest.mark.parametrize("with_public", [False, True])
def test_prove_mixed(gpu, with_public):
    hs = [_handle(gpu, name, seed) for name, seed, _ in JOB]
    try:
        groups = []
        for (name, seed, n), h in zip(JOB, hs):
            pub = None
            inputs = _inputs(name, n, b"job")
            if with_public and name == "bin_test":
                pub = [(-1) ** j * (j % 9) for j in range(n)]
                inputs = _binary_net_inputs(pub, 11)
            groups.append((h, inputs, _prefixes(n, name.encode()), pub))
        got = RP.prove_mixed(gpu, groups)
        assert [len(g) for g in got] == [n for _, _, n in JOB]
        # every group: the files of prove_batch_pub on a fresh handle
        for (name, seed, n), (h, inputs, prefixes, pub), files in zip(JOB, groups, got):
            ref = _handle(gpu, name, seed)
            try:
                assert ref.prove_batch(inputs, prefixes, public_amounts=pub) == files, name
            finally:
                ref.close()
        # one table for the family — over the longest basis among its non-empty groups —, the unrelated setup's own, none for the empty group
        infos = [h.comb_info() for h in hs]
        related = [i for i, (_, seed, n) in enumerate(JOB) if seed is None and n]
        longest = max(_basis_len(hs[i]) for i in related)
        for i in related:
            assert infos[i] == infos[related[0]] and infos[i]["users"] == len(related) and infos[i]["points"] == longest
        assert infos[3]["users"] == 0
        assert infos[6]["users"] == 1 and infos[6]["points"] == _basis_len(hs[6])
        if with_public:
            h, _, _, pub = groups[5]
            assert h.verify_batch([c for c, _ in got[5]], [p for _, p in got[5]], SEED, public_amounts=pub)
        else:
            assert RP.verify_mixed(gpu, [(h, [c for c, _ in f], [p for _, p in f]) for h, f in zip(hs, got)], SEED)
        # a second job on the same handles keeps the table and the bytes
        again = RP.prove_mixed(gpu, groups[:3])
        assert again == got[:3] and hs[0].comb_info() == infos[0]
    finally:
        for h in hs:
            h.close()


def test_prove_mixed_refusals(gpu):
    import bulletproofspp_amd as b
    a, c = _handle(gpu, "32bit"), _handle(gpu, "64bit")
    ctx2 = b.Bppp(0)
    far = _handle(ctx2, "64bit")
    try:
        ga = (a, _inputs("32bit", 2), _prefixes(2))
        with pytest.raises(BpppError) as e:
            RP.prove_mixed(gpu, [ga, (c, _inputs("64bit", 1), _prefixes(1)), ga])
        assert "(-1)" in str(e.value) and "group 2" in str(e.value) and "two groups" in str(e.value)
        with pytest.raises(BpppError) as e:
            RP.prove_mixed(gpu, [ga, (far, _inputs("64bit", 1), _prefixes(1))])
        assert "(-1)" in str(e.value) and "group 1" in str(e.value) and "contexts" in str(e.value)
        bad = _inputs("32bit", 3)
        bad[2] = [(2**40, ty, bl) for _, ty, bl in bad[2]]          # outside [0, 2^32): the message names the group and the proof
        with pytest.raises(BpppError) as e:
            RP.prove_mixed(gpu, [(c, _inputs("64bit", 1), _prefixes(1)), (a, bad, _prefixes(3))])
        assert "(-1)" in str(e.value) and "group 1" in str(e.value) and "proof 2" in str(e.value)
        assert RP.prove_mixed(gpu, []) == [] and RP.prove_mixed(gpu, [(a, [], [])]) == [[]]
        assert RP.prove_mixed(gpu, [ga])[0] == a.prove_batch(ga[1], ga[2])      # still usable
    finally:
        a.close(); c.close(); far.close(); ctx2.close()


# ----------------------------------------------------------------------------- 7. verify_each over a borrowed table
def test_verify_each_over_a_borrowed_table(gpu, donors):
    borrower, plain = _handle(gpu, "32by64"), _handle(gpu, "32by64")
    try:
        borrower.share_comb(donors["128by64"])
        files = borrower.prove_batch(_inputs("32by64", 4), _prefixes(4))
        coms, proofs = [c for c, _ in files], [p for _, p in files]
        bad = bytearray(proofs[2]); bad[7] ^= 4
        proofs[2] = bytes(bad)
        assert plain.comb_info()["users"] == 0       # never proved: decides over the windowed table of its basis
        want = plain.verify_each(coms, proofs, want_points=True)
        got = borrower.verify_each(coms, proofs, want_points=True)
        assert got == want and got[0] == [0, 0, 1, 0] and got[1][2] is not None
    finally:
        borrower.close(); plain.close()
