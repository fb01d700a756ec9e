"""The pair forms of the Fq multiplication (csrc/fq26.hip.h: fq_mul2, fq_mul_sqr, fq_sqr2 — two independent products issued as four
interleaved carry chains, for the kernels that walk a chain of point additions on a lone wavefront) against fq_mul / fq_sqr, raw 26-bit
limbs bit for bit, and against the integers: the value of every result is the product mod p and its limbs have magnitude 1.  Operands are
raw limbs built here: random canonical values, the edge set of benchmarks/fe26_model.py (0, 1, p - 1, every limb at the magnitude-8
bound), each pair in both orders, and pairs that share an operand."""
import random

import numpy as np
import pytest

from bulletproofspp_amd.capi import load_test_library

pytestmark = pytest.mark.gpu

P = 2**256 - 2**32 - 977
M26, M22 = (1 << 26) - 1, (1 << 22) - 1
MAG8 = [2 * 8 * M26] * 9 + [2 * 8 * M22]            # rand_mag(extreme=True) of benchmarks/fe26_model.py at m = 8
KINDS = {"mul2": 0, "mul_sqr": 1, "sqr2": 2}


def _limbs(x):
    return [(x >> (26 * i)) & M26 for i in range(10)]


def _val(l):
    return sum(int(v) << (26 * i) for i, v in enumerate(l))


@pytest.fixture(scope="module")
def operands():
    """(a, b, c, d) limb rows: 4096 random quadruples, then the edge set in every position, both orders, shared operands"""
    rnd = random.Random(2611)
    rows = [tuple(_limbs(rnd.randrange(P)) for _ in range(4)) for _ in range(4096)]
    edge = [_limbs(0), _limbs(1), _limbs(P - 1), MAG8]
    r1, r2 = _limbs(rnd.randrange(P)), _limbs(rnd.randrange(P))
    for x in edge:
        for y in edge:
            rows.append((x, y, r1, r2))          # the edge product first, a random one beside it
            rows.append((r1, r2, x, y))          # ... and second
            rows.append((x, y, y, x))            # the same product on both sides, operands swapped
            rows.append((x, y, x, r1))           # a shared left operand
            rows.append((r1, x, y, x))           # a shared right operand
    for _ in range(64):                          # random magnitudes up to 8 on all four, and shared operands
        q = [[rnd.randrange(2 * 8 * M26 + 1) for _ in range(9)] + [rnd.randrange(2 * 8 * M22 + 1)] for _ in range(4)]
        rows.append(tuple(q))
        rows.append((q[0], q[1], q[1], q[0]))
        rows.append((q[0], q[1], q[0], q[2]))
    arr = np.array(rows, dtype=np.uint32)        # [n, 4, 10]
    return [np.ascontiguousarray(arr[:, k, :]) for k in range(4)]


@pytest.mark.parametrize("kind", list(KINDS))
def test_pair_forms_equal_single_products_limb_for_limb(gpu, operands, kind):
    a, b, c, d = operands
    n = a.shape[0]
    raw = np.zeros((n, 40), dtype=np.uint32)
    rc = load_test_library().bppp_test_fq_pair(gpu.h, KINDS[kind], a.ctypes.data, b.ctypes.data, c.ctypes.data, d.ctypes.data, n, raw.ctypes.data)
    assert rc == 0, gpu.lib.bppp_last_error(gpu.h)
    bad = np.flatnonzero((raw[:, :20] != raw[:, 20:]).any(axis=1))
    assert bad.size == 0, f"{kind}: pair and single limbs differ at rows {bad[:8].tolist()}"
    # magnitude 1 out, and the right residue
    assert (raw[:, 0:9] <= 2 * M26).all() and (raw[:, 10:19] <= 2 * M26).all() and (raw[:, 9] <= 2 * M22).all() and (raw[:, 19] <= 2 * M22).all()
    for i in range(n):
        va, vb, vc, vd = _val(a[i]), _val(b[i]), _val(c[i]), _val(d[i])
        w1 = va * va if kind == "sqr2" else va * vb
        w2 = vc * vd if kind == "mul2" else vc * vc
        assert _val(raw[i, :10]) % P == w1 % P and _val(raw[i, 10:20]) % P == w2 % P, (kind, i)
