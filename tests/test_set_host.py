"""The hashlib restatements of the set commitments in rangeproof.py (set_leaf_host, set_peaks_host, set_root_host, set_path_host,
set_verify_path_host: the reference of every GPU test in tests/test_gpu_set.py) against a naive recursive definition written here from the text of
include/bppp.h: node (k, j) by recursion over its two children, the peaks from the set bits of n, the bag, the root and the path by their
definitions.  Any split of the rows into appends gives the same peaks and root; every leaf's path verifies; every single changed place gets the
verdict the definition gives; h + p + 1 <= bit_length (n) for all n < 2^14; the root of the empty set."""
import functools
import hashlib
import random

from bulletproofspp_amd import rangeproof as RP

TAG = b"host set"
H = lambda *parts: hashlib.sha256(b"".join(parts)).digest()
D = {part: H(b"bppp/set/" + part + b"/v1", TAG) for part in (b"leaf", b"node", b"bag", b"root")}
NROWS = 600
ROWS = [bytes(random.Random(i).randrange(256) for _ in range(33)) for i in range(NROWS)]


@functools.lru_cache(maxsize=None)
def node(k, j):
    """node (k, j) over ROWS, by the definition"""
    return H(D[b"leaf"], ROWS[j]) if k == 0 else H(D[b"node"], node(k - 1, 2 * j), node(k - 1, 2 * j + 1))


def naive_peaks(n):
    return [node(k, ((n >> (k + 1)) << (k + 1)) >> k) for k in range(n.bit_length() - 1, -1, -1) if (n >> k) & 1]


def naive_bag(peaks):
    if not peaks:
        return bytes(32)
    acc = peaks[-1]
    for i in range(len(peaks) - 2, -1, -1):
        acc = H(D[b"bag"], peaks[i], acc)
    return acc


def naive_root(n, rb=33):
    return H(D[b"root"], n.to_bytes(8, "little"), rb.to_bytes(4, "little"), naive_bag(naive_peaks(n)))


def naive_where(n, i):
    """(h, p, first leaf of the peak) of leaf i"""
    start = 0
    for p, k in enumerate(k for k in range(n.bit_length() - 1, -1, -1) if (n >> k) & 1):
        if i < start + (1 << k):
            return k, p, start
        start += 1 << k
    return None


def naive_path(n, i):
    h, p, _ = naive_where(n, i)
    peaks = naive_peaks(n)
    out = [node(s, (i >> s) ^ 1) for s in range(h)]
    if p < len(peaks) - 1:
        out.append(naive_bag(peaks[p + 1:]))
    out += [peaks[q] for q in range(p - 1, -1, -1)]
    assert len(out) <= n.bit_length()
    return b"".join(out) + bytes(32 * (n.bit_length() - len(out)))


def naive_verdict(n, root, i, row, path, rb=33):
    if i >= n:
        return RP.SET_BAD_INDEX
    h, p, _ = naive_where(n, i)
    m = bin(n).count("1")
    used = h + p + (1 if p < m - 1 else 0)
    if path[32 * used:] != bytes(len(path) - 32 * used):
        return RP.SET_BAD_PADDING
    acc = H(D[b"leaf"], row)
    for s in range(h):
        sib = path[32 * s:32 * s + 32]
        acc = H(D[b"node"], sib, acc) if (i >> s) & 1 else H(D[b"node"], acc, sib)
    s = h
    if p < m - 1:
        acc = H(D[b"bag"], acc, path[32 * s:32 * s + 32])
        s += 1
    for _ in range(p):
        acc = H(D[b"bag"], path[32 * s:32 * s + 32], acc)
        s += 1
    return RP.SET_OK if H(D[b"root"], n.to_bytes(8, "little"), rb.to_bytes(4, "little"), acc) == root else RP.SET_MISMATCH


def test_the_domains_and_the_leaf():
    assert RP._set_domain(b"leaf", TAG) == D[b"leaf"] and RP.set_leaf_host(TAG, ROWS[3]) == node(0, 3)
    assert RP.set_leaf_host(b"", b"\x01") == hashlib.sha256(hashlib.sha256(b"bppp/set/leaf/v1").digest() + b"\x01").digest()


def test_peaks_and_roots_equal_the_definition():
    for n in range(NROWS + 1):
        peaks = RP.set_peaks_host(TAG, ROWS[:n])
        assert peaks == naive_peaks(n), n
        assert RP.set_root_host(TAG, 33, n, peaks) == naive_root(n), n
    assert RP.set_root_host(TAG, 33, 0, []) == H(D[b"root"], bytes(8), (33).to_bytes(4, "little"), bytes(32))
    assert RP.set_root_host(TAG, 34, 5, naive_peaks(5)) != naive_root(5) and RP.set_root_host(TAG, 34, 5, naive_peaks(5)) == naive_root(5, 34)


def test_any_split_into_appends_gives_the_same_state():
    rnd = random.Random(11)
    for trial in range(60):
        n = rnd.randrange(NROWS + 1) if trial else NROWS
        cuts = sorted(rnd.randrange(n + 1) for _ in range(rnd.randrange(6)))
        state, at = (0, []), 0
        for c in cuts + [n]:
            state = (c, RP.set_peaks_host(TAG, ROWS[at:c], start=state))
            at = c
        assert state[1] == naive_peaks(n), (n, cuts)
        assert RP.set_root_host(TAG, 33, n, state[1]) == naive_root(n)


def test_every_leafs_path_is_the_definitions_and_verifies():
    for n in [1, 2, 3, 4, 5, 7, 8, 77, 255, 256, 257, 511, 600]:
        levels, root = RP.set_levels_host(TAG, ROWS[:n]), naive_root(n)
        assert all(levels[k][j] == node(k, j) for k in range(len(levels)) for j in range(len(levels[k])))
        for i in range(n):
            path = RP.set_path_host(TAG, ROWS[:n], i, levels)
            assert path == naive_path(n, i) and len(path) == RP.set_path_bytes(n) == 32 * n.bit_length(), (n, i)
            assert RP.set_verify_path_host(TAG, 33, n, root, i, ROWS[i], path) == RP.SET_OK == naive_verdict(n, root, i, ROWS[i], path)
    assert RP.set_path_host(TAG, ROWS[:9], 8) == naive_path(9, 8)


def _flip(bs, o, bit=1):
    return bs[:o] + bytes([bs[o] ^ bit]) + bs[o + 1:]


def test_every_single_changed_place_gets_the_definitions_verdict():
    rnd = random.Random(3)
    seen = set()
    for n in [1, 2, 3, 6, 77, 300, 600]:
        root = naive_root(n)
        for i in sorted({0, n - 1, n // 2, rnd.randrange(n)}):
            row, path = ROWS[i], naive_path(n, i)
            h, p, _ = naive_where(n, i)
            used = 32 * (h + p + (1 if p < bin(n).count("1") - 1 else 0))
            cases = [(n, root, i, _flip(row, o, 1 << rnd.randrange(8)), path) for o in range(33)]
            cases += [(n, root, i, row, _flip(path, o, 1 << rnd.randrange(8))) for o in range(len(path))]
            cases += [(n, root, j, row, path) for j in set(range(max(0, i - 3), i + 4)) | {n - 1, n, n + 1, 2**63} if j != i]
            cases += [(n, _flip(root, o), i, row, path) for o in range(32)]
            for n2 in {n - 1, n + 1, n ^ 1, n ^ 2, 2 * n, n + 2**40} - {0, n}:
                pb = RP.set_path_bytes(n2)
                cases.append((n2, root, i, row, path[:pb].ljust(pb, b"\0")))
            for k, (n_, root_, i_, row_, path_) in enumerate(cases):
                want = naive_verdict(n_, root_, i_, row_, path_)
                assert RP.set_verify_path_host(TAG, 33, n_, root_, i_, row_, path_) == want, (n, i, k)
                seen.add(want)
                if n_ == n and root_ == root and i_ == i and row_ == row:      # a changed path byte: used bytes mismatch, padding bytes are named
                    o = next(o for o in range(len(path)) if path_[o] != path[o])
                    assert want == (RP.SET_MISMATCH if o < used else RP.SET_BAD_PADDING)
                elif n_ == n and i_ == i:
                    assert want == RP.SET_MISMATCH                              # a row byte or a root byte
    assert seen == {RP.SET_MISMATCH, RP.SET_BAD_INDEX, RP.SET_BAD_PADDING} or seen == {RP.SET_OK, RP.SET_MISMATCH, RP.SET_BAD_INDEX, RP.SET_BAD_PADDING}


def test_the_length_always_suffices():
    for n in range(1, 2**14):
        levels = RP._set_peak_levels(n)
        assert max(h + p + 1 for p, h in enumerate(levels)) <= n.bit_length(), n
        assert [RP._set_locate(n, sum(1 << k for k in levels[:p]))[:2] for p in range(len(levels))] == [(h, p) for p, h in enumerate(levels)] if n < 2**9 else True
