"""Jobs for the cut-through tests (tests/test_cut_through_host.py, tests/test_gpu_cut_through.py): commitments files made of byte strings — no curve
is needed, the call never lifts a point — and the hand-made and seeded random jobs both test files run.  A job is a dict: nranges, rows (files),
sum_start, entries, claims (None or one (amount, type, offset) per sum)."""
import random

from bulletproofspp_amd import rangeproof as rp

P, N = rp.FIELD_P, rp.N
ADD, SUB = False, True


def put(x: int) -> bytes:
    """Binary (Prime p) put: four 64-bit limbs, least significant first, each big-endian"""
    return b"".join(((x >> (64 * i)) & (2**64 - 1)).to_bytes(8, "big") for i in range(4))


def row(xs, signs=0, pad=0) -> bytes:
    """a commitments file of len(xs) ranges: the sign bytes (bit i = sign of commitment i; pad fills the unused bits of the last byte), then put (x)"""
    nr = len(xs)
    bits = signs | (pad << nr)
    return bits.to_bytes((nr + 7) // 8, "little")[: (nr + 7) // 8] + b"".join(put(x) for x in xs)


def x_of(name) -> int:
    """a fixed x below p - 2^200 for a name, so that x + p still fits 256 bits only where a test wants it to"""
    return int.from_bytes(__import__("hashlib").sha256(repr(name).encode()).digest(), "big") % (2**255)


def job(nranges, rows, txs, claims=None):
    """txs: one list of (flat index, subtract) per transaction"""
    start, entries = [0], []
    for tx in txs:
        entries += [rp.tally_entry(j, s) for j, s in tx]
        start.append(len(entries))
    return dict(nranges=nranges, rows=rows, sum_start=start, entries=entries, claims=claims)


def widen(j, nr):
    """a one-range job on a handle of nr <= 8 ranges: every row gets nr - 1 commitments of its own behind the one it had (never referenced, never
    equal to anything), the padding bits move up, and entry index r becomes r * nr"""
    assert j["nranges"] == 1 and nr <= 8
    rows = [bytes([(f[0] & 1) | (((f[0] >> 1) << nr) & 0xFF)]) + f[1:] + b"".join(put(x_of(("wide", r, i))) for i in range(1, nr)) for r, f in enumerate(j["rows"])]
    entries = [(e & rp.TALLY_SUBTRACT) | ((e & (rp.TALLY_SUBTRACT - 1)) * nr) for e in j["entries"]]
    return dict(j, nranges=nr, rows=rows, entries=entries)


A, B, C, D = (x_of(n) for n in "ABCD")
SMALL = 5                                                    # an x with x + p below 2^256


def hand_made():
    """name -> job, one range a row unless the name says otherwise"""
    r1 = lambda x, s=0, pad=0: row([x], s, pad)
    jobs = {}
    # tx1 spends A, makes B; tx2 spends (its copy of) B, makes C; tx3 spends C, makes D: - A + D is left
    jobs["chain"] = job(1, [r1(A), r1(B), r1(B), r1(C), r1(C), r1(D)], [[(0, SUB), (1, ADD)], [(2, SUB), (3, ADD)], [(4, SUB), (5, ADD)]])
    jobs["inside_one_tx"] = job(1, [r1(A), r1(B), r1(B)], [[(0, SUB), (1, ADD), (2, SUB)]])
    jobs["two_outputs_one_spend"] = job(1, [r1(B), r1(B), r1(B)], [[(0, ADD)], [(1, ADD)], [(2, SUB)]])
    jobs["three_outputs_one_spend"] = job(1, [r1(B), r1(B), r1(B), r1(B)], [[(0, ADD)], [(1, ADD)], [(2, ADD)], [(3, SUB)]])
    jobs["double_spend"] = job(1, [r1(A), r1(A), r1(C)], [[(0, SUB), (2, ADD)], [(1, SUB)]])
    jobs["x_plus_p"] = job(1, [r1(SMALL), r1(SMALL + P)], [[(0, ADD)], [(1, SUB)]])
    jobs["sign_differs"] = job(1, [r1(B, 0), r1(B, 1)], [[(0, ADD)], [(1, SUB)]])
    jobs["padding_differs"] = job(1, [r1(B, 1, pad=0), r1(B, 1, pad=0x55)], [[(0, ADD)], [(1, SUB)]])
    jobs["same_index_both_signs"] = job(1, [r1(A), r1(B)], [[(0, ADD), (1, ADD)], [(0, SUB)]])
    # nothing is cut: the outputs (rows 1 and 3) go in front of the inputs (rows 0 and 2)
    jobs["row_order"] = job(1, [r1(A), r1(B), r1(C), r1(D)], [[(0, SUB), (1, ADD)], [(2, SUB), (3, ADD)]])
    # B is made once and spent once (row 1 and row 5 go); D is made once and spent twice through one row: the second spend survives
    jobs["mixed_counts"] = job(1, [r1(A), r1(B), r1(C), r1(D), r1(D), r1(B)], [[(2, SUB), (0, ADD), (1, ADD)], [(3, ADD), (4, SUB), (4, SUB), (5, SUB)]])
    jobs["claims"] = job(1, [r1(A), r1(B), r1(B), r1(C)], [[(0, SUB), (1, ADD)], [(2, SUB), (3, ADD)]],
                         claims=[(-7, 3, N - 2), (2, N - 1, 5)])
    jobs["claims_wrap"] = job(1, [r1(A), r1(B)], [[(0, ADD)], [(1, ADD)]], claims=[(N - 1, 1, N - 1), (N - 1, N - 1, 2)])
    return jobs


def hand_made_two_ranges():
    r2 = lambda x0, x1, s=0, pad=0: row([x0, x1], s, pad)
    jobs = {}
    # row 0 = (A, B) made by tx 1; tx 2 spends B alone through its copy (row 1): row 0 stays whole and is an output (A survives added);
    # row 1 is gone
    jobs["half_spent_output"] = job(2, [r2(A, B), r2(C, B, pad=1)], [[(0, ADD), (1, ADD)], [(3, SUB)]])
    # row 0 = (A, B) is spent in both halves, but only B's creation is in the set: row 0 survives for - A and is NOT an output
    jobs["half_spent_input"] = job(2, [r2(A, B), r2(D, B)], [[(0, SUB), (1, SUB)], [(3, ADD), (2, ADD)]])
    jobs["signs_per_range"] = job(2, [r2(A, A, 0b01), r2(A, A, 0b10)], [[(0, ADD), (1, ADD)], [(2, SUB), (3, SUB)]])
    return jobs


def random_job(seed, nnz, nranges=1, spent=0.3, claims=True):
    """a seeded job of exactly nnz entries: outputs with fresh identities, about `spent` of them spent inside the set by a later (or earlier)
    transaction through a row of its own, and some identities repeated up to 5 times on either side"""
    rnd = random.Random(seed)
    rows, txs, tx = [], [], []
    pool = []                                               # identities (x, sign) created so far
    n = 0

    def ref(x, sign, sub):
        nonlocal n
        if nranges == 1 or not rows or rnd.random() < 0.5 or rows[-1][2] >= nranges:
            rows.append([[x] + [x_of(("fill", seed, len(rows), i)) for i in range(nranges - 1)], sign, 1])
            j = (len(rows) - 1) * nranges
        else:                                               # the next free range of the last row
            r = rows[-1]
            i = r[2]
            r[0][i] = x
            r[1] = (r[1] & ~(1 << i)) | (sign << i)
            r[2] += 1
            j = (len(rows) - 1) * nranges + i
        tx.append((j, sub))
        n += 1

    while n < nnz:
        u = rnd.random()
        if pool and u < spent:
            x, s = rnd.choice(pool)
            for _ in range(rnd.choice([1, 1, 1, 1, 2, 5])):
                if n < nnz:
                    ref(x + P if x + P < 2**256 and rnd.random() < 0.5 else x, s, SUB)
        elif u < spent + 0.1:
            ref(x_of(("in", seed, n)), rnd.randrange(2), SUB)
        else:
            x, s = x_of(("out", seed, n)) >> rnd.choice([0, 0, 0, 230]), rnd.randrange(2)
            pool.append((x, s))
            for _ in range(rnd.choice([1, 1, 1, 1, 1, 3, 5])):
                if n < nnz:
                    ref(x, s, ADD)
        if rnd.random() < 0.4:
            txs.append(tx)
            tx = []
    txs.append(tx)
    if rnd.random() < 0.5:
        rnd.shuffle(txs)                                    # a spend may come before its output
    files = [row(xs, s, pad=rnd.randrange(4)) for xs, s, _ in rows]
    cl = [(rnd.randrange(-2**40, 2**40), rnd.randrange(N), rnd.randrange(N)) for _ in txs] if claims else None
    return job(nranges, files, txs, cl)


def one_identity(nnz, alternate):
    """nnz entries of one identity through two rows of equal content: signs alternating, or all added"""
    files = [row([B], 1), row([B], 1, pad=3)]
    return job(1, files, [[(k & 1, bool(k & 1) if alternate else ADD)] for k in range(nnz)])
