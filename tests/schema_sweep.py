"""A seeded sweep of range-proof schemas: the structure the range-proof layer branches on, sampled instead of hand-picked.

A plain helper module (no fixture, no pytest setting).  `sweep()` returns the same list on every call and every machine: random.Random over
fixed string seeds, nothing else.  tests/test_schema_sweep_host.py pins what the list covers and that the host protocol code proves and
verifies every member; tests/test_gpu_schema_sweep.py compares the native layer with the host code on each.

One entry (`Schema`):
  name      unique
  binary    RangeProof.Binary (True) or RangeProof.TypedReciprocal (False)
  ranges    reciprocal: (base, lo, hi, shared, output, assumed); binary: (lo, hi, output, assumed)
  cons      reciprocal: typed (the amounts of the one type balance); binary: conserved (always: BRP.witness demands it)
  pubs      the public amounts [(isOutput, type, amount)]; a binary setup's net public amount is their signed sum
  ty        the type of every ranged amount (0 on an untyped setup)
  flavour   "NL" or "IP"
  wits      three rows of amounts: every range at its minimum, every range at max - 1 — both as far as the balance allows, the first
            ranges that can move make up the difference —, and random in-range values (an assumed range takes whatever is left over)

Only setups the library documents as accepted are built: every reciprocal width is at least its base (a width of 2 .. base - 1 is refused,
NARROW below), every inline range has at least (1 if it has a leading bit) + base - 1 digits (csrc/rpsetup.hpp make_setup), assumed ranges
appear only under types or conservation.  Size limits keep a GPU case to seconds: nrm_len <= 48, lin_len <= 40; a candidate beyond them is
discarded and counted (`discarded()`).  The one exception is stated where it is made: the binary setup that holds the 2^64-wide range
the sweep must contain has that range alone, 64 norm positions.

The four coefficient forms of makeRangeData (TypedReciprocal.hs:103-120) for a width w, n1 = integerLog base (w - 1):
  "power"      no leading bit, w = base^(n1 + 1)
  "plain"      no leading bit ((w - 1) divisible by base - 1), w not a power
  "bit"        a leading bit, w < 2 base^n1
  "bit+digit"  a leading bit and the extra digit bn1"""
import dataclasses
import random
from typing import List, Tuple

import pyoracle as O
from bulletproofspp_amd import rangeproof as RP
from bulletproofspp_amd import rangeproof_binary as BRP

N = O.N
SEED = "schema sweep 1"
MAX_NRM, MAX_LIN = 48, 40
BASES = (2, 3, 4, 5, 6, 7, 8, 11, 16)
FORMS = ("power", "plain", "bit", "bit+digit")
N_RECIPROCAL, N_BINARY = 32, 12
# (base, width): refused by bppp_rp_create ("range narrower than its digit base"), shared and inline; the first widths accepted beside them
NARROW = [(3, 2), (4, 3), (10, 5), (16, 10), (16, 15)]
TYPES = (15, 7, 1, 2**200 + 5)


@dataclasses.dataclass
class Schema:
    name: str
    binary: bool
    ranges: list
    cons: bool
    pubs: List[Tuple[bool, int, int]]
    ty: int
    flavour: str
    wits: List[List[int]]

    @property
    def net_public(self):
        return sum(-v if io else v for io, _, v in self.pubs)


# ----------------------------------------------------------------------------- widths of a given coefficient form
def form_of(base, w):
    n1 = RP.integer_log(base, w - 1)
    if (w - 1) % (base - 1) == 0:
        return "power" if w == base ** (n1 + 1) else "plain"
    return "bit" if w < 2 * base ** n1 else "bit+digit"


def digit_count(form, n1):
    return n1 + 2 if form == "bit+digit" else n1 + 1


def inline_min_n1(base, form):
    """the least n1 at which an inline range has (1 if bit) + base - 1 digits; never below the least n1 the form exists at"""
    need = base - 1 + (1 if form.startswith("bit") else 0)
    return max(need - (2 if form == "bit+digit" else 1), form_min_n1(base, form))


def form_min_n1(base, form):
    return 0 if form == "power" else 1


def width_of(rnd, base, form, n1):
    """a width of that form with integerLog base (w - 1) = n1: drawn in the form's interval, then the next member of the form upwards (cyclic)"""
    p = base ** n1
    if form == "power":
        return p * base
    lo, hi = {"plain": (p + 1, p * base - 1), "bit": (p + 1, 2 * p - 1), "bit+digit": (2 * p, p * base - 1)}[form]
    assert lo <= hi, (base, form, n1)
    w = rnd.randrange(lo, hi + 1)
    for _ in range(2 * base + 2):
        if form_of(base, w) == form:
            return w
        w = lo if w == hi else w + 1
    raise AssertionError("no width of form %s for base %d at n1 = %d" % (form, base, n1))


def usable_form(base, form):
    """base 2 has no leading bit (every w - 1 is divisible by 1): its ranges are "power" or "plain\""""
    return form if base > 2 or not form.startswith("bit") else "plain"


# ----------------------------------------------------------------------------- balance
def _bounds(ranges_loh):
    """per range (sign, lo, hi - 1, assumed) -> the interval of its contribution sign * v"""
    return [((lo, hi1) if sg > 0 else (-hi1, -lo)) for sg, lo, hi1, _ in ranges_loh]


def balance(rows, target, net):
    """amounts closest to `target` (in range order) with net + sum sign_i v_i = 0: an assumed range absorbs everything (it is never checked);
    without one the first ranges that can move take the difference.  None if the ranges cannot balance `net` at all."""
    c = [sg * v for (sg, _, _, _), v in zip(rows, target)]
    rest = -net - sum(c)
    for i, (sg, _, _, assumed) in enumerate(rows):
        if assumed:
            c[i] += rest
            rest = 0
            break
    for i, (a, b) in enumerate(_bounds(rows)):
        if rows[i][3] or not rest:
            continue
        s = max(a - c[i], min(b - c[i], rest))
        c[i] += s
        rest -= s
    if rest:
        return None
    return [sg * x for (sg, _, _, _), x in zip(rows, c)]


def _rows_of(ranges, binary):
    if binary:
        return [(-1 if out else 1, lo, hi - 1, asm) for lo, hi, out, asm in ranges]
    return [(-1 if out else 1, lo, hi - 1, asm) for _, lo, hi, _, out, asm in ranges]


def _witnesses(rnd, rows, net, balanced):
    """the three rows of amounts; with `balanced` None when the ranges cannot meet `net`"""
    rand = [rnd.randrange(lo, hi1 + 1) for _, lo, hi1, _ in rows]
    targets = [[lo for _, lo, _, _ in rows], [hi1 for _, _, hi1, _ in rows], rand]
    if not balanced:
        return targets
    out = [balance(rows, t, net) for t in targets]
    return None if any(w is None for w in out) else out


def _publics(rnd, rows, kind, ty):
    """a public list of the wanted kind (0: none, 1: one amount, 2: an input, an output and a cancelling pair) that the ranges can balance,
    and its net amount.  Kind 0 falls back to kind 1 where the ranges alone cannot reach zero."""
    if kind == 0 and balance(rows, [lo for _, lo, _, _ in rows], 0) is not None:
        return [], 0
    rand = [rnd.randrange(lo, hi1 + 1) for _, lo, hi1, _ in rows]
    net = -sum(sg * v for (sg, _, _, _), v in zip(rows, rand))
    if kind != 2:
        return [(net < 0, ty, abs(net))], net
    other = TYPES[(TYPES.index(ty) + 1) % len(TYPES)] if ty in TYPES else ty
    pair = rnd.randrange(1, 2**40)
    b = rnd.randrange(1, 1000) + max(-net, 0)                      # input a = net + b >= 1, output b
    pubs = [(False, ty, net + b), (True, other, pair), (True, ty, b), (False, other, pair)]
    if rnd.random() < 0.5:                                         # the pair in the ranges' own type, three entries
        pubs = [(False, ty, pair), (net < 0, ty, abs(net)), (True, ty, pair)]
    return pubs, net


# ----------------------------------------------------------------------------- reciprocal candidates
# ranges of the directed members: (base, form, shared, n1 or None = drawn, assumed); the rest of such a member is drawn like any other
DIRECTED = {
    0: (False, [(2, "plain", True, None, False), (5, "bit", True, None, False)]),           # 2 enters m_bases from both sides
    1: (False, [(4, "bit", False, 3, False)]),                                             # inline, symbols = digits exactly (1 + 3 = 4)
    2: (False, [(3, "power", False, None, False), (4, "plain", False, None, False), (5, "power", True, None, False), (7, "plain", True, None, False)]),
    3: (True, [(6, "bit+digit", False, 4, False), (3, "bit", True, None, False), (8, "plain", True, None, True)]),      # symbols = digits (1 + 5 = 6)
    4: (False, [(4, "power", True, 0, False)]),                                             # width = base: one digit, one base
    5: (True, [(16, "bit+digit", True, None, False), (11, "bit", True, None, False), (2, "power", True, None, True)]),
}
MINIMA = ("0", "1", "10", "-20", "-w", "2^64")


def _minimum(kind, w):
    return {"0": 0, "1": 1, "10": 10, "-20": -20, "-w": -w, "2^64": 2**64}[kind]


def _reciprocal_candidate(i):
    rnd = random.Random("%s reciprocal %d" % (SEED, i))
    typed, plan = DIRECTED.get(i, (i % 2 == 1, None))
    flavour = "NL" if (i // 2) % 2 == 0 else "IP"
    nr = len(plan) if plan else rnd.randrange(1, 5)
    room = (MAX_NRM + 8) // nr                                     # digits a range may take: loose on purpose, the size check below decides
    lin_left = MAX_LIN - 6
    ranges = []
    for j in range(nr):
        if plan:
            base, form, shared, n1, assumed = plan[j]
        else:
            form, shared = FORMS[(i + j) % 4], ((i // 4) + j) % 2 == 0
            if j:
                form, shared = rnd.choice(FORMS), rnd.random() < 0.5
            assumed = typed and j > 0 and rnd.random() < 0.3
            if shared:
                fits = [b for b in BASES if b - 1 <= lin_left - 1]
                shared = bool(fits)
            if not shared:
                fits = [b for b in BASES if digit_count(usable_form(b, form), inline_min_n1(b, usable_form(b, form))) <= room]
            base, n1 = rnd.choice(fits), None
        form = usable_form(base, form)
        n_lo = form_min_n1(base, form) if shared else inline_min_n1(base, form)
        if n1 is None:
            n_hi = max(n_lo, room - (2 if form == "bit+digit" else 1))
            n1 = rnd.randrange(n_lo, n_hi + 1) if rnd.random() < 0.7 else n_lo
        w = width_of(rnd, base, form, n1)
        assert form_of(base, w) == form and w >= base
        lo = _minimum(MINIMA[(i + 2 * j) % len(MINIMA)], w)
        if shared and not assumed:
            lin_left -= base - 1
        ranges.append((base, lo, lo + w, shared, rnd.random() < 0.5, assumed))
    rows = _rows_of(ranges, False)
    ty = TYPES[i % len(TYPES)] if typed else 0
    pubs, net = _publics(rnd, rows, (i // 2) % 3, ty) if typed else ([], 0)
    wits = _witnesses(rnd, rows, net, typed)
    return Schema("r%02d-%s-%s-%s" % (i, flavour, "typed" if typed else "untyped", "-".join("%d%s%s" % (b, "s" if sh else "i", "a" if asm else "")
                                                                                             for b, _, _, sh, _, asm in ranges)),
                  False, ranges, typed, pubs, ty, flavour, wits)


# ----------------------------------------------------------------------------- binary candidates
BIN_WIDTHS = ("1", "2", "3", "2^k", "2^k+1", "2^64", "any")
BIN_MINIMA = (0, 3, -7, 2**40)


def _binary_candidate(i):
    rnd = random.Random("%s binary %d" % (SEED, i))
    flavour = "NL" if i % 2 == 0 else "IP"
    nr = 1 if i == 5 else rnd.randrange(1, 5)                      # i = 5 draws the 2^64-wide range: alone, the one member above MAX_NRM
    room = MAX_NRM // nr
    ranges = []
    for j in range(nr):
        kind = BIN_WIDTHS[(i + 3 * j) % len(BIN_WIDTHS)]
        k = rnd.randrange(1, room)
        w = {"1": 1, "2": 2, "3": 3, "2^k": 2**k, "2^k+1": 2**k + 1, "2^64": 2**64, "any": rnd.randrange(2**(k - 1) + 1, 2**k + 1)}[kind]
        if w == 2**64 and nr > 1:
            w = 2**k
        lo = BIN_MINIMA[(i + j) % len(BIN_MINIMA)]
        ranges.append((lo, lo + w, rnd.random() < 0.5, j > 0 and rnd.random() < 0.3))
    rows = _rows_of(ranges, True)
    pubs, net = _publics(rnd, rows, i % 2, 0)
    wits = _witnesses(rnd, rows, net, True)
    return Schema("b%02d-%s-%s" % (i, flavour, "-".join("%d%s" % (RP.integer_log(2, hi - lo - 1) + 1, "a" if asm else "") for lo, hi, _, asm in ranges)),
                  True, ranges, True, pubs, 0, flavour, wits)


# ----------------------------------------------------------------------------- the host setups and the sweep
_POINTS = []


def points():
    if not _POINTS:
        _POINTS.extend(O.hash_points(b"schema sweep", 4 + MAX_LIN + 64))
    return _POINTS


def range_data(s):
    mk = BRP.make_range_data if s.binary else RP.make_range_data
    rds = [mk(*r) for r in s.ranges]
    assert all(rd is not None for rd in rds)
    return rds


def basis_points_needed(s, rds):
    """the points `setup` takes for this schema, by its own arithmetic (TypedReciprocal.hs:332-359: h, g, linLen, nrmLen; Binary.hs:147-148: h, g,
    h0, h1, nrmLen): a norm position per coefficient of every range and one per range under types; six linear positions and base - 1 per
    distinct shared base of the live ranges, 2 among them when a live shared range has a leading bit"""
    if s.binary:
        return 4 + sum(len(rd.base_coeffs) for rd in rds)
    live = [rd for rd in rds if not rd.is_assumed]
    m_bases = {rd.base for rd in live if rd.is_shared} | ({2} if any(rd.has_bit and rd.is_shared for rd in live) else set())
    return 2 + 6 + sum(b - 1 for b in m_bases) + sum(len(rd.base_coeffs) + (1 if s.cons else 0) for rd in rds)


def host_setup(backend, s):
    rds = range_data(s)
    need = basis_points_needed(s, rds)
    pts = points() if need <= len(points()) else size_points(need)      # every member of the sweep fits points(); the size edges may not
    if s.binary:
        return BRP.setup(backend, pts, s.cons, rds, s.net_public, s.flavour)
    return RP.setup(backend, pts, s.cons, list(s.pubs), rds, s.flavour)


def _fits(s):
    st = host_setup(RP.Backend(), s)
    if s.binary and len(s.ranges) == 1 and s.ranges[0][1] - s.ranges[0][0] == 2**64:
        return st.nrm_len == 64
    return st.nrm_len <= MAX_NRM and st.lin_len <= MAX_LIN


_SWEEP = {}


def _generate():
    if _SWEEP:
        return
    kept, candidates, dropped = [], 0, 0
    for count, make in ((N_RECIPROCAL, _reciprocal_candidate), (N_BINARY, _binary_candidate)):
        i, have = 0, 0
        while have < count:
            s = make(i)
            i += 1
            candidates += 1
            if s.wits is None or not _fits(s):
                dropped += 1
                continue
            kept.append(s)
            have += 1
    assert len({s.name for s in kept}) == len(kept)
    _SWEEP.update(kept=kept, candidates=candidates, dropped=dropped)


def sweep():
    """the kept setups, reciprocal ones first"""
    _generate()
    return list(_SWEEP["kept"])


def discarded():
    """(candidates discarded for a size limit or for ranges that cannot balance, candidates drawn)"""
    _generate()
    return _SWEEP["dropped"], _SWEEP["candidates"]


def edge_setups():
    """the first two widths bppp_rp_create accepts beside NARROW's (4, 3): base 4 over [0, 4) (one digit of coefficient 1) and over [0, 5)
    (a leading bit, coefficients [1, 1]) — shared (an inline base-4 range needs three digits), untyped, both flavours between them"""
    out = []
    for w, flavour in ((4, "NL"), (5, "IP")):
        out.append(Schema("edge-base4-width%d-%s" % (w, flavour), False, [(4, 0, w, True, True, False)], False, [], 0, flavour, [[0], [w - 1], [1]]))
    return out


def by_name(name):
    s = next((s for s in sweep() + edge_setups() if s.name == name), None)
    return s if s is not None else next(s for s in size_edges() if s.name == name)


# ----------------------------------------------------------------------------- the setup size classes of the native layer
# Setups that sit on the edges where the native range-proof layer changes its path with the SIZE of a setup (tests/test_size_classes_host.py
# pins what they cover, tests/test_gpu_size_classes.py runs them): the 16 slots of the base map, the reciprocal-symbol limit, the classes of
# the prover's reciprocal table, the 64 KiB and 160 KiB edges of the dynamic LDS of k_rpp_phase2, k_rpp_phase3 and k_trrp_public, the
# prover's wide-table clause and the binary range limit.  The range counts at the LDS edges are not written down here: they are found by
# bisection on bppp_test_rp_lds_plan, the functions that size the launches themselves, and `size_expect()` says which class every member
# was built for — a test that finds it elsewhere fails and says that the shape must be picked again.
MAX_SLOTS, MAX_SYMS, MAX_BINARY_RANGES, MAX_RANGES = 16, 1022, 1024, 65535
LDS_DEFAULT, LDS_MAX = 64 * 1024, 160 * 1024
K_PUBLIC, K_PHASE2, K_PHASE3 = 0, 2, 3
WIDE_TYPE = 2**200
_SIZE = {}
_SIZE_POINTS = []
_TLIB = []


def lds_plan(kernel, max_base=0, nranges=0, nsyms=0, batch=1):
    """bppp_test_rp_lds_plan: the planned dynamic LDS of one launch (no GPU, no context)"""
    import ctypes as C
    from bulletproofspp_amd import capi
    if not _TLIB:
        _TLIB.append(capi.load_test_library())
    r = capi.TestRpLdsPlan()
    assert _TLIB[0].bppp_test_rp_lds_plan(kernel, max_base, nranges, nsyms, batch, C.byref(r)) == 0
    return r


def first_count(pred, hi=1 << 20):
    """the least n in [1, hi] with pred(n), for a monotone pred: bisection"""
    lo = 1
    assert pred(hi)
    while lo < hi:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


def lds_edges():
    """the range counts at which a setup of inline base-2 ranges (table class 16, one reciprocal symbol) changes class"""
    if "edges" not in _SIZE:
        p2 = lambda n: lds_plan(K_PHASE2, 2, n).lds_bytes
        p3 = lambda n: lds_plan(K_PHASE3, 2, n).lds_bytes
        pub = lambda n: lds_plan(K_PUBLIC, 0, n, 1, 1).lds_bytes
        _SIZE["edges"] = dict(
            phase2_64k=first_count(lambda n: p2(n) > LDS_DEFAULT), phase3_64k=first_count(lambda n: p3(n) > LDS_DEFAULT),
            public_64k=first_count(lambda n: pub(n) > LDS_DEFAULT), phase2_max=first_count(lambda n: p2(n) > LDS_MAX) - 1,
            public_max=first_count(lambda n: pub(n) > LDS_MAX) - 1)
    return dict(_SIZE["edges"])


def size_points(n):
    """the first n points of the size-edge basis (a prefix of one stream: a longer request extends it)"""
    if len(_SIZE_POINTS) < n:
        _SIZE_POINTS[:] = O.hash_points(b"schema sweep size edges", next((m for m in (1200, 4200) if m >= n), n))
    return _SIZE_POINTS[:n]


def _untyped(name, ranges, flavour="NL"):
    rnd = random.Random("%s size %s" % (SEED, name))
    rows = _rows_of(ranges, False)
    return Schema(name, False, ranges, False, [], 0, flavour, _witnesses(rnd, rows, 0, False))


def _typed(name, ranges, kind, ty, more_pubs=()):
    """typed with public amounts: the ranges' own type balanced as the sweep balances it, `more_pubs` (pairs that cancel) in front"""
    rnd = random.Random("%s size %s" % (SEED, name))
    rows = _rows_of(ranges, False)
    pubs, net = _publics(rnd, rows, kind, ty)
    wits = _witnesses(rnd, rows, net, True)
    assert wits is not None
    return Schema(name, False, ranges, True, list(more_pubs) + pubs, ty, "NL", wits)


def _bases16():
    """bases 2 .. 17, no leading bit anywhere (every width a power of its base): inline 2, 3 and 14 (1, 2 and 13 digits), the rest shared with
    one digit — slot 12 (base 14) inline, slots 13 .. 15 (15, 16, 17) shared"""
    out = []
    for b in range(2, 18):
        inline = b in (2, 3, 14)
        out.append((b, 0, b ** (b - 1) if inline else b, not inline, b % 2 == 1, False))
    return out


def _many(n):
    return [(2, 0, 2, False, i % 2 == 1, False) for i in range(n)]


def _generate_size_edges():
    if "list" in _SIZE:
        return
    out, exp = [], {}

    def put(s, **e):
        out.append(s)
        exp[s.name] = dict(dict(refused=None, binary=False), **e)

    e = lds_edges()
    # a, b: the base map's slots
    a = _bases16()
    for s in (_untyped("size-a-bases16-untyped-NL", a), _typed("size-a-bases16-typed-NL", a, 2, TYPES[0]), _untyped("size-a-bases16-untyped-IP", a, "IP")):
        put(s, slots=16, table=32, nsyms=16 + (len({t for _, t, _ in s.pubs} - set(range(1, 17)))), prove="device", lds2="default", lds3="default", public="default")
    put(_untyped("size-b-bases17-untyped-NL", a + [(18, 0, 18, True, False, False)]), slots=17, nsyms=17,
        refused=["17 distinct digit bases", "at most 16"])
    # c: the classes of the prover's reciprocal table, one shared one-digit range (its top digit base - 1 reads the table's last live entry)
    for b, table in ((16, 16), (17, 32), (256, 256), (257, 512), (512, 512), (513, 1024), (1023, 1024)):
        put(_untyped("size-c-base%d-shared" % b, [(b, 0, b, True, True, False), (4, 0, 4, True, False, False)]), slots=2, table=table, nsyms=b - 1, prove="device",
            lds2="above" if table == 1024 else "default", lds3="default", public="default")      # 1024 reciprocals alone pass 64 KiB in phase 2
    # an ASSUMED range has no digits and no symbols: its base, however wide, neither widens the table nor takes a slot or the host algebra
    put(_typed("size-c-base4-beside-assumed-base2000", [(4, 0, 4, True, False, False), (2000, 0, 2000, True, True, True)], 1, TYPES[0]), slots=1, table=16,
        nsyms=4, prove="device", lds2="default", lds3="default", public="default")
    # d: the reciprocal-symbol limit
    put(_untyped("size-d-base1024-shared", [(1024, 0, 1024, True, True, False), (4, 0, 4, True, False, False)]), slots=2, nsyms=1023,
        refused=["1023 reciprocal symbols", "at most 1022"])
    d = [(1000, 0, 1000, True, False, False), (4, 0, 4, True, True, True)]          # the assumed range takes what the public amounts leave
    for extra, name in ((MAX_SYMS - 999 - 1, "size-d-base1000-typed-at-the-limit"), (MAX_SYMS - 999, "size-d-base1000-typed-one-over")):
        pairs = [(io, WIDE_TYPE + 7 * k, 1000 + k) for k in range(1, extra + 1) for io in (False, True)]
        s = _typed(name, d, 1, WIDE_TYPE, pairs)
        n = 999 + len({t for _, t, _ in s.pubs})
        if n <= MAX_SYMS:
            put(s, slots=1, table=1024, nsyms=n, prove="device", lds2="above", lds3="default", public="default")
        else:
            put(s, slots=1, nsyms=n, refused=["%d" % n, "reciprocal symbols", "at most 1022"])
    # e: a wide table (base above 256) with 256 and with 257 ranges: the prover's second clause
    for n, route in ((256, "device"), (257, "host")):
        put(_untyped("size-e-base257-%dranges" % n, [(257, 0, 257, True, i % 2 == 1, False) for i in range(n)]), slots=1, table=512, nsyms=256, prove=route,
            lds2="default", lds3="default", public="default")
    # f: many small ranges around the 64 KiB edges
    big = max(e["phase2_64k"], e["phase3_64k"], e["public_64k"]) + 50
    n3 = e["phase3_64k"]
    assert max(e["phase2_64k"], e["public_64k"]) <= n3 - 1 and big <= e["phase2_max"]      # else: pick these shapes again
    put(_untyped("size-f-%dranges-below-phase3-64k" % (n3 - 1), _many(n3 - 1)), slots=1, table=16, nsyms=1, prove="device", lds2="above", lds3="default", public="above")
    put(_untyped("size-f-%dranges-above-phase3-64k" % n3, _many(n3)), slots=1, table=16, nsyms=1, prove="device", lds2="above", lds3="above", public="above")
    put(_untyped("size-f-%dranges-above-all-64k" % big, _many(big)), slots=1, table=16, nsyms=1, prove="device", lds2="above", lds3="above", public="above")
    put(_typed("size-f-%dranges-above-all-64k-typed" % big, _many(big), 1, TYPES[0]), slots=1, table=16, nsyms=2, prove="device", lds2="above", lds3="above",
        public="above")
    # g: the last range count the device algebra serves, and the first it does not
    g = e["phase2_max"]
    put(_untyped("size-g-%dranges-prover-limit" % g, _many(g)), slots=1, table=16, nsyms=1, prove="device", lds2="above", lds3="above", public="above")
    put(_untyped("size-g-%dranges-past-prover-limit" % (g + 1), _many(g + 1)), slots=1, table=16, nsyms=1, prove="host", lds2="over", lds3="above", public="above")
    # h: the last nsyms + nr the one-kernel verifier serves, and the first it does not
    h = e["public_max"]
    assert h > g + 1
    put(_untyped("size-h-%dranges-verifier-limit" % h, _many(h)), slots=1, table=16, nsyms=1, prove="host", lds2="over", lds3="above", public="above")
    put(_untyped("size-h-%dranges-past-verifier-limit" % (h + 1), _many(h + 1)), slots=1, table=16, nsyms=1, prove="host", lds2="over", lds3="above", public="three")
    # i: the binary range limit
    for n in (MAX_BINARY_RANGES, MAX_BINARY_RANGES + 1):
        rnd = random.Random("%s size binary %d" % (SEED, n))
        ranges = [(0, 2, i % 2 == 1, False) for i in range(n)]
        rows = _rows_of(ranges, True)
        pubs, net = _publics(rnd, rows, 0, 0)
        put(Schema("size-i-binary-%dranges" % n, True, ranges, True, pubs, 0, "NL", _witnesses(rnd, rows, net, True)), binary=True,
            refused=None if n <= MAX_BINARY_RANGES else ["%d ranges" % n, "at most 1024 ranges"])
    assert len({s.name for s in out}) == len(out) and all(s.wits is not None and len(s.wits) == 3 for s in out)
    _SIZE.update(list=out, expect=exp)


def size_edges():
    """the setups at the native layer's size-class edges (not part of sweep()); the same list on every machine"""
    _generate_size_edges()
    return list(_SIZE["list"])


def size_expect(name):
    """what a size-edge member was built for:
      refused   None, or the pieces of bppp_rp_create's message
      slots     distinct digit bases (the base map's slots in use)
      table     the class of the prover's reciprocal table (16 .. 1024)
      nsyms     reciprocal symbols
      prove     the route a default prove takes: "device" algebra or "host" algebra
      lds2/3    the dynamic LDS of k_rpp_phase2 / k_rpp_phase3: "default" (<= 64 KiB), "above" (64 KiB .. 160 KiB), "over" (does not fit)
      public    k_trrp_public for a batch of at most 1024 proofs: "default", "above", or "three" (the three-kernel route instead)"""
    _generate_size_edges()
    return dict(_SIZE["expect"][name])


# ----------------------------------------------------------------------------- proofs (seeded as tests/test_few_rounds_host.py::inputs_of)
def inputs_of(s, amounts, seed):
    """the prover's rows for one proof: (amount, blinding) per binary range, (amount, type, blinding) per reciprocal one"""
    rnd = random.Random("schema sweep blinding %s %r" % (s.name, seed))
    if s.binary:
        return [(v, rnd.randrange(N)) for v in amounts]
    return [(v, s.ty, rnd.randrange(N)) for v in amounts]


def prefix_of(j):
    return b"schema sweep proof %d" % j


def host_prove(st, s, j):
    """the host protocol's proof of witness j"""
    mod = BRP if s.binary else RP
    return mod.prove(st, mod.witness(st, inputs_of(s, s.wits[j], j)), RP.sha256_oracle(), RP.hash_to_scalar(prefix_of(j)))
