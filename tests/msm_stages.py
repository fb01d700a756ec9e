"""Helpers of the tests that read the stages of an MSM back (bppp_test_last_msm_layout / _copy, include/bppp_test.h): the layout as a dict, the arrays
as numpy arrays, contexts created under a tuning environment, and k_digits restated on the digit format of test_gpu_msm_reduce_known_logs.Fmt (the
stored 16-bit digit and the sign-mask bit of a scalar, where Fmt.digits gives the signed digit they amount to).  Not a test module."""
import ctypes

import numpy as np
import pytest

import pyoracle as O

N = O.N
LAYOUT_FIELDS = ("c", "W", "acnt", "top", "M", "flat", "CH", "Q", "one_read", "sized", "fq29", "L", "shared_points", "stride", "per", "batch", "n", "FB", "G", "total",
                 "table_stride")
U64P = ctypes.POINTER(ctypes.c_uint64)


def layout(g):
    from bulletproofspp_amd.capi import TestMsmLayout, load_test_library
    rep = TestMsmLayout()
    rc = load_test_library().bppp_test_last_msm_layout(g.h, ctypes.byref(rep))
    assert rc == 0, g.lib.bppp_last_error(g.h)
    return {f: int(getattr(rep, f)) for f in LAYOUT_FIELDS}


def read(g, lay, what):
    """one array of the last MSM: digits [batch * W][stride] u16, negmask bits [batch * n] bool, count [FB], start [FB + 1], sorted [total] u32, raw [FB][40] u32,
    aff [FB][16] u32"""
    from bulletproofspp_amd import capi
    NB = lay["batch"] * lay["W"]
    words = -(-lay["batch"] * lay["n"] // 64)
    code, dtype, shape = {"digits": (capi.TEST_MSM_DIGITS, np.uint16, (NB, lay["stride"])), "negmask": (capi.TEST_MSM_NEGMASK, np.uint64, (words,)),
                          "count": (capi.TEST_MSM_COUNT, np.uint32, (lay["FB"],)), "start": (capi.TEST_MSM_START, np.uint32, (lay["FB"] + 1,)),
                          "sorted": (capi.TEST_MSM_SORTED, np.uint32, (lay["total"],)), "raw": (capi.TEST_MSM_BUCKETS_RAW, np.uint32, (lay["FB"], 40)),
                          "aff": (capi.TEST_MSM_BUCKETS_AFF, np.uint32, (lay["FB"], 16))}[what]
    out = np.zeros(shape, dtype=dtype)
    rc = capi.load_test_library().bppp_test_last_msm_copy(g.h, code, out.ctypes.data, out.nbytes)
    assert rc == 0, g.lib.bppp_last_error(g.h)
    if what == "negmask":
        return np.unpackbits(out.view(np.uint8), bitorder="little")[:lay["batch"] * lay["n"]].astype(bool), out
    return out


def hooks(g):
    """(bucket ranges Q, k_scatter_one_read, sized, fq29) of the last general-pipeline MSM, by the bppp_test_last_* hooks"""
    from bulletproofspp_amd.capi import load_test_library
    lib, out = load_test_library(), []
    for f in (lib.bppp_test_last_sort_ranges, lib.bppp_test_last_scatter_one_read, lib.bppp_test_last_acc_sized, lib.bppp_test_last_acc_fq29):
        v = ctypes.c_int(-2)
        assert f(g.h, ctypes.byref(v)) == 0
        out.append(v.value)
    return tuple(out)


def make_contexts(gpu, envs):
    """env (a sorted tuple of (name, value)) -> context created under it, the environment restored; () is the session's context"""
    import bulletproofspp_amd as b
    made = {(): gpu}
    for env in sorted(set(envs) - {()}):
        with pytest.MonkeyPatch.context() as mp:
            for k in ("BPPP_SORT_RANGES", "BPPP_SCATTER_ONE_READ", "BPPP_HIST_CH", "BPPP_LACC", "BPPP_ACC_SIZED", "BPPP_ACC_FQ29"):
                mp.delenv(k, raising=False)
            for k, v in env:
                mp.setenv(k, v)
            made[env] = b.Bppp(0)
    return made


def close_contexts(made):
    for env, g in made.items():
        if env:
            g.close()


def recode(fmt, rows):
    """k_digits on the restated format: (stored [batch][W][n] uint16, neg [batch][n] bool); every digit is tied to Fmt.digits, the signed digit that
    the consumers make of the stored one, the sign-mask bit and the flip of the top row"""
    batch, n = len(rows), len(rows[0])
    stored = np.zeros((batch, fmt.W, n), dtype=np.uint16)
    neg = np.zeros((batch, n), dtype=bool)
    for b, row in enumerate(rows):
        for j, s in enumerate(row):
            ng = s > N - s
            sp = (N - s if ng else s) + fmt.K
            sig = fmt.digits(s)
            for w in range(fmt.W):
                cw = fmt.cw[w]
                f = sp & ((1 << cw) - 1)
                sp >>= cw
                st = fmt.M - f if w == fmt.top else f + (0 if w < fmt.acnt else 1 << (fmt.c - 2))
                kv = st - fmt.M
                assert 0 <= st < 1 << 16 and sig[w] == (-abs(kv) if (kv < 0) ^ ng ^ (w == fmt.top) else abs(kv))
                stored[b, w, j] = st
            assert sp == 0
            neg[b, j] = ng
    return stored, neg


def entries(fmt, stored, neg, flat, CH, per, table_stride):
    """what the sort must make of the stored digits: per non-zero digit its flat bucket fb, the rank of its run inside the bucket (the chunk, or for a
    registered basis (window, chunk): the order the cursors of k_count_tiles give the runs) and its 4-byte entry sign << 31 | index; sorted by
    (bucket, run, entry)"""
    batch, W, n = stored.shape
    M = fmt.M
    kv = stored.astype(np.int64) - M
    b, w, j = np.nonzero(kv)
    v = kv[b, w, j]
    sign = (v < 0) ^ neg[b, j] ^ (w == fmt.top)
    fb = ((b if flat else b * W + w) * M + np.abs(v) - 1).astype(np.int64)
    ch = j // per
    assert ch.size == 0 or ch.max() < CH
    run = (w * CH + ch if flat else ch).astype(np.int64)
    ent = (sign.astype(np.int64) << 31) | (w * table_stride + j if flat else j)
    o = np.lexsort((ent, run, fb))
    return fb[o], run[o], ent[o]


def observed_runs(sorted_, count, flat, CH, per, table_stride):
    """(bucket, run, entry) of every position of `sorted`, the run derived from the entry's own index"""
    fb = np.repeat(np.arange(count.size, dtype=np.int64), count.astype(np.int64))
    ent = sorted_.astype(np.int64)
    idx = ent & 0x7FFFFFFF
    if flat:
        run = (idx // table_stride) * CH + (idx % table_stride) // per
    else:
        run = idx // per
    return fb, run, ent


def collapsed_oracle(ec, base, scalars, index):
    """the oracle's sum s_i B_(index_i) over the few base points: the scalars of one base point are added up as integers first"""
    tot = [0] * len(base)
    for s, k in zip(scalars, index):
        tot[k] += s
    return ec.inner_product([(t % N, p) for t, p in zip(tot, base) if t % N])
