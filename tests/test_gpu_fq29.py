"""csrc/fq29.hip.h (Fq in 9 x 29-bit limbs, the field type of k_acc_points_sized29) through bppp_test_fq29_op, on raw limbs built here:
every result equals the bit-exact model (benchmarks/fe29_model.py) limb for limb and the integers canonically; fq29_to_fq26 gives limbs
below 2^26 and from_fe -> to_fq26 round-trips.  Operands: 0, 1, p - 1, p - 2^32, all 29-bit limbs ones, single bits and runs around the
32 -> 29 repacking borders, every limb at the maximum of its magnitude, and 4 096 random pairs."""
import importlib.util
import os
import random

import numpy as np
import pytest

from bulletproofspp_amd.capi import load_test_library

pytestmark = pytest.mark.gpu

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "benchmarks", "fe29_model.py")
_spec = importlib.util.spec_from_file_location("fe29_model", _PATH)
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

P = M.P
OPS = {"mul": 0, "sqr": 1, "sub_weak": 2, "from_fe": 3}


def _border_values():
    """single bits, and runs of ones ending, at every 29-bit and 32-bit boundary below 2^256"""
    out = []
    for k in sorted({29 * i for i in range(1, 9)} | {32 * j for j in range(1, 8)}):
        out += [1 << (k - 1), 1 << k, (1 << k) - 1, (1 << (k + 1)) - 1, ((1 << 256) - (1 << k)) % P, (3 << (k - 1)) % P]
    return out


def _edge_canonical():
    return [0, 1, P - 1, P - 2**32, 2, 977, 2**32, 2**255] + _border_values()


def _run(gpu, op, a, b):
    a = np.ascontiguousarray(np.array(a, dtype=np.uint32)); b = np.ascontiguousarray(np.array(b, dtype=np.uint32))
    n = a.shape[0]
    raw = np.zeros((n, 19), dtype=np.uint32); out = np.zeros((n, 8), dtype=np.uint32)
    rc = load_test_library().bppp_test_fq29_op(gpu.h, OPS[op], a.ctypes.data, b.ctypes.data, n, raw.ctypes.data, out.ctypes.data)
    assert rc == 0, gpu.lib.bppp_last_error(gpu.h)
    return raw, out


def _canon(words):
    return sum(int(w) << (32 * i) for i, w in enumerate(words))


def _check(op, a, b, raw, out, want_limbs, want_value):
    for i in range(len(a)):
        got = [int(x) for x in raw[i, :9]]
        assert got == want_limbs[i], (op, i, a[i], b[i])
        assert [int(x) for x in raw[i, 9:]] == M.to_fq26(want_limbs[i]), (op, i)
        assert _canon(out[i]) == want_value[i] % P, (op, i)
    assert (raw[:, 9:] < (1 << 26)).all()


@pytest.fixture(scope="module")
def pairs():
    """(tight a, b of magnitude <= 7) limb rows"""
    rnd = random.Random(2929)
    edge = [M.from_int(v) for v in _edge_canonical()] + [[M.M29] * 8 + [M.M24], M.mag_limbs(1), M.PL]
    rows = [(M.from_int(rnd.randrange(P)), M.from_int(rnd.randrange(P))) for _ in range(4096)]
    r = M.from_int(rnd.randrange(P))
    for x in edge:
        rows += [(x, r), (r, x), (x, x), (x, M.mag_limbs(7)), (x, M.PL)]
    for x in edge[:12]:
        for y in edge[:12]:
            rows.append((x, y))
    rows.append((M.mag_limbs(1), M.mag_limbs(7)))
    for m in (2, 3, 5, 7):
        for _ in range(64):
            rows.append((M.rand_mag(rnd, 1), M.rand_mag(rnd, m)))
    for _ in range(64):
        rows.append((M.rand_mag(rnd, 2), M.rand_mag(rnd, 3)))
    return rows


def test_mul(gpu, pairs):
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    raw, out = _run(gpu, "mul", a, b)
    _check("mul", a, b, raw, out, [M.mul(x, y) for x, y in pairs], [M.val(x) * M.val(y) for x, y in pairs])


def test_mul_is_symmetric_in_its_contract(gpu, pairs):
    """the loose operand on the left"""
    sel = pairs[-200:]
    a, b = [p[1] for p in sel], [p[0] for p in sel]
    raw, out = _run(gpu, "mul", a, b)
    _check("mul", a, b, raw, out, [M.mul(x, y) for x, y in zip(a, b)], [M.val(x) * M.val(y) for x, y in zip(a, b)])


def test_sqr(gpu, pairs):
    rnd = random.Random(5)
    a = [p[0] for p in pairs] + [M.mag_limbs(1), M.mag_limbs(2)] + [M.rand_mag(rnd, 2) for _ in range(256)]
    raw, out = _run(gpu, "sqr", a, a)
    _check("sqr", a, a, raw, out, [M.sqr(x) for x in a], [M.val(x) ** 2 for x in a])


def test_sub_then_weak_pass(gpu, pairs):
    rnd = random.Random(6)
    rows = [(x, y) for x, y in pairs if M.mag_ok(y, 3)]
    rows += [(M.mag_limbs(3), M.mag_limbs(3)), (M.mag_limbs(3), [0] * 9), ([0] * 9, M.mag_limbs(3)), (M.PL, M.PL), ([0] * 9, [0] * 9)]
    rows += [(M.rand_mag(rnd, 3), M.rand_mag(rnd, 3)) for _ in range(512)]
    a, b = [p[0] for p in rows], [p[1] for p in rows]
    raw, out = _run(gpu, "sub_weak", a, b)
    want = [M.weak_pass(M.sub(x, y, 3)) for x, y in rows]
    _check("sub_weak", a, b, raw, out, want, [M.val(x) - M.val(y) for x, y in rows])
    assert (raw[:, :8] < (1 << 29)).all() and (raw[:, 8] <= (1 << 24) + 7).all()


def test_from_fe_and_back_round_trips(gpu):
    rnd = random.Random(7)
    vals = _edge_canonical() + [rnd.randrange(P) for _ in range(4096)]
    a = [[(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0] for v in vals]
    raw, out = _run(gpu, "from_fe", a, a)
    for i, v in enumerate(vals):
        assert [int(x) for x in raw[i, :9]] == M.from_int(v), (i, hex(v))
        assert sum(int(x) << (26 * j) for j, x in enumerate(raw[i, 9:])) == v, (i, hex(v))
        assert _canon(out[i]) == v
    assert (raw[:, 9:] < (1 << 26)).all()
