"""CPU checks of the outlier filters (dicp_amd/filter.py) that need no GPU.

``dicp_amd/csrc/dicp_filter.h`` -- the rules the HIP kernels execute -- is compiled with g++ through tests/hostcheck/filter_check.cpp and
held to tests/filter_ref.py bit for bit: sum64, the slot rule, the mean distances, the statistics and the decision; the same comparison is
shown to refuse five wrong rules.  The argument checks of the three functions run before any device work, and every class of bad call of
the new entry points of libdicp_hip.so gives its status code without launching.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import _lib
from dicp_amd import filter as F
from dicp_amd.filter import radius_outlier_removal, select_rows, statistical_outlier_removal

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostbuild  # noqa: E402
import filter_ref as fr  # noqa: E402
from ball_ref import d2_matrix  # noqa: E402

RIGHT, SEQUENTIAL, POPULATION, STRICT, KEEP_SELF, FUSED, KERNEL_ROUNDS = range(7)
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def fc():
    lib = hostbuild.build("filter_check.cpp", "filter_check")
    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    lib.fc_constants.argtypes, lib.fc_constants.restype = [vp], None
    lib.fc_levels.argtypes, lib.fc_levels.restype = [i64], i32
    lib.fc_level_len.argtypes, lib.fc_level_len.restype = [i64, i32], i64
    lib.fc_sum64.argtypes, lib.fc_sum64.restype = [vp, i64, i32], f64
    for fn in (lib.fc_row_means_f32, lib.fc_row_means_f64):
        fn.argtypes, fn.restype = [vp, vp, i32, i32, i32, vp, vp], None
    for fn in (lib.fc_cloud_f32, lib.fc_cloud_f64):
        fn.argtypes, fn.restype = [vp, vp, i32, i32, i32, f64, i32, vp, vp, vp], None
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _bits(x):
    return np.float64(x).tobytes()


def _sum64(fc, v, variant=RIGHT):
    v = np.ascontiguousarray(v, dtype=np.float64)
    return fc.fc_sum64(_p(v), v.size, variant)


def _cloud(fc, d2, idx, k, ratio, rows=None, variant=RIGHT):
    d2, idx = np.ascontiguousarray(d2), np.ascontiguousarray(idx, dtype=np.int64)
    m = d2.shape[0]
    md, stats, mask = np.zeros(m, np.float64), np.zeros(3, np.float64), np.zeros(m, np.uint8)
    fn = fc.fc_cloud_f32 if d2.dtype == np.float32 else fc.fc_cloud_f64
    fn(_p(d2), _p(idx), m, m if rows is None else rows, k, float(ratio), variant, _p(md), _p(stats), _p(mask))
    return md, stats, mask.astype(bool)


def _same(got, ref):
    return all(fr.same_bits(a, b) for a, b in zip(got, ref))


def knn_brute(x, k1):
    """the k1 nearest rows of x for every row of x in (d2, index) order, as knn_points defines them -> d2 (m, k1), idx (m, k1) int64"""
    m = x.shape[0]
    D = d2_matrix(x[:, :3], x[:, :3])
    d2 = np.full((m, k1), np.inf, dtype=x.dtype)
    idx = np.full((m, k1), -1, dtype=np.int64)
    for i in range(m):
        j = np.flatnonzero(np.isfinite(D[i]))
        j = j[np.argsort(D[i, j], kind="stable")][:k1]
        d2[i, :j.size], idx[i, :j.size] = D[i, j], j
    return d2, idx


def random_cloud(m, dtype, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((m, 3)).astype(dtype)


def synthetic_search(m, k, dtype, seed=0):
    """a search result written down directly (no distance matrix): row i finds itself at 0, then rows i + 1 ... at ascending distances"""
    rng = np.random.default_rng(seed)
    idx = (np.arange(m)[:, None] + np.arange(k + 1)[None, :]) % m
    d2 = np.sort(rng.random((m, k + 1)), axis=1).astype(dtype)
    d2[:, 0] = 0
    d2[::50, 1:] *= 30                                                # some rows far from everything
    return d2, idx.astype(np.int64)


# ------------------------------------------------------------------ the header against the reference
def test_constants_match_the_module(fc):
    c = np.zeros(5, np.int32)
    fc.fc_constants(_p(c))
    assert list(c) == [F.SELECT_TILE, F.SELECT_SCAN_THREADS, fr.CHUNK, F.K_MIN, F.K_MAX]
    assert [fc.fc_levels(n) for n in (1, 64, 65, 4096, 4097, 262144, 262145)] == [1, 1, 2, 2, 3, 3, 4]
    assert [fc.fc_level_len(n, 1) for n in (0, 1, 64, 65, 4097)] == [0, 1, 1, 2, 65]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4096, 4097, 4096 * 64 + 65])
def test_sum64(fc, n):
    rng = np.random.default_rng(n)
    v = rng.random(n) * 10.0 ** rng.integers(-3, 4, n)
    ref = fr.sum64(v)
    assert _bits(_sum64(fc, v)) == _bits(ref)
    assert _bits(_sum64(fc, v, KERNEL_ROUNDS)) == _bits(ref)          # the kernels' rounds, one more than needed: the same value
    assert _sum64(fc, np.zeros(0)) == 0.0


def test_sum64_is_not_the_sequential_sum(fc):
    rng = np.random.default_rng(3)
    v = rng.random(4097)
    tree, plain = fr.sum64(v), fr.sum64(v, tree=False)
    assert tree != plain                                              # (the data: a length and values on which the two orders differ)
    assert _bits(_sum64(fc, v)) == _bits(tree)
    assert _bits(_sum64(fc, v, SEQUENTIAL)) == _bits(plain) != _bits(tree)


@pytest.mark.parametrize("dtype", DTYPES)
def test_slot_rule(fc, dtype):
    k = 3
    rows = {                                                          # row number -> its k + 1 slots
        5: [5, 1, 2, 3],                                              # self in slot 0
        6: [1, 2, 6, 3],                                              # self in a middle slot, behind exact duplicates
        7: [1, 2, 3, 4],                                              # self absent: the first k
        8: [8, 1, -1, -1],                                            # a -1 tail
        9: [-1, -1, -1, -1],                                          # nothing
    }
    m = 10
    idx = np.full((m, k + 1), -1, dtype=np.int64)
    d2 = np.full((m, k + 1), np.inf, dtype=dtype)
    for i, slots in rows.items():
        idx[i] = slots
        d2[i] = np.array([0.0, 0.0, 0.3, 0.7], dtype=dtype)
        d2[i][np.array(slots) < 0] = np.inf
    md, cnt = np.zeros(m), np.zeros(m, np.int32)
    (fc.fc_row_means_f32 if dtype == np.float32 else fc.fc_row_means_f64)(_p(d2), _p(idx), m, k, RIGHT, _p(md), _p(cnt))
    ref = [fr.row_mean(d2[i], idx[i], i, k) for i in range(m)]
    assert fr.same_bits(md, np.array([r[0] for r in ref])) and list(cnt) == [r[1] for r in ref]
    assert [int(cnt[i]) for i in (5, 6, 7, 8, 9)] == [3, 3, 3, 1, 0] and md[9] == np.inf and md[8] == 0.0
    a, b = np.sqrt(np.float64(dtype(0.3))), np.sqrt(np.float64(dtype(0.7)))
    assert md[5] == ((0.0 + a) + b) / 3 and md[7] == ((0.0 + 0.0) + a) / 3 and md[6] == ((0.0 + 0.0) + b) / 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_clouds(fc, dtype):
    k = 2
    # V = 0: one row, which finds only itself
    d2, idx = knn_brute(np.zeros((1, 3), dtype), k + 1)
    got = _cloud(fc, d2, idx, k, 2.0)
    assert _same(got, fr.outlier_ref(d2, idx, k, 2.0)) and not got[2].any() and got[0][0] == np.inf and np.isnan(got[1][0]) and got[1][1] == 0.0
    # V = 1: a row with a neighbour, a row without (its coordinates are not finite)
    x = np.array([[0.0, 0, 0], [1.0, 0, 0], [np.nan, 0, 0]], dtype)
    d2, idx = knn_brute(x, k + 1)
    d2[1], idx[1] = np.inf, -1
    got = _cloud(fc, d2, idx, k, 2.0)
    assert _same(got, fr.outlier_ref(d2, idx, k, 2.0)) and list(got[2]) == [True, False, False] and list(got[1]) == [1.0, 0.0, 1.0]
    # V = 2
    d2, idx = knn_brute(np.array([[0.0, 0, 0], [0.5, 0, 0]], dtype), k + 1)
    got = _cloud(fc, d2, idx, k, 0.0)
    assert _same(got, fr.outlier_ref(d2, idx, k, 0.0)) and got[2].all() and list(got[1]) == [0.5, 0.0, 0.5]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,k,rows", [(300, 8, None), (300, 8, 200), (70, 31, None), (4200, 1, 4199)])
def test_random_cloud(fc, dtype, m, k, rows):
    if m > 4096:                                                      # (three rounds of sum64)
        d2, idx = synthetic_search(rows, k, dtype)
    else:
        x = random_cloud(m, dtype, seed=m + k)
        dup = np.arange(0, m - 1, 37)
        x[dup] = x[dup + 1]                                           # exact duplicates
        x[5, 1] = np.nan
        d2, idx = knn_brute(x[:rows], k + 1)
    if rows is not None:                                              # pad rows: empty slots
        d2 = np.concatenate([d2, np.full((m - rows, k + 1), np.inf, dtype)])
        idx = np.concatenate([idx, np.full((m - rows, k + 1), -1, np.int64)])
    ref = fr.outlier_ref(d2, idx, k, 1.5, rows=rows)
    assert 0 < ref[2].sum() < (rows or m)
    assert _same(_cloud(fc, d2, idx, k, 1.5, rows=rows), ref)
    assert _same(_cloud(fc, d2, idx, k, 1.5, rows=rows, variant=KERNEL_ROUNDS), ref)


# ------------------------------------------------------------------ the comparison refuses wrong rules
@pytest.fixture(scope="module")
def plain_cloud():
    """500 random rows on which the wrong summation rules show in the statistics: picked by running the rules side by side in numpy"""
    for seed in range(20):
        d2, idx = knn_brute(random_cloud(500, np.float64, seed=seed), 9)
        ref = fr.outlier_ref(d2, idx, 8, 1.0)
        if all(fr.outlier_ref(d2, idx, 8, 1.0, **kw)[1][1] != ref[1][1] for kw in ({"tree": False}, {"fused": True})):
            return d2, idx, ref
    raise AssertionError("no seed separates the rules")


def test_refuses_a_sequential_sum(fc, plain_cloud):
    d2, idx, ref = plain_cloud
    wrong = fr.outlier_ref(d2, idx, 8, 1.0, tree=False)
    assert not fr.same_bits(wrong[1], ref[1])                         # (500 rows: the tree and the plain order give other statistics)
    assert _same(_cloud(fc, d2, idx, 8, 1.0), ref)
    assert _same(_cloud(fc, d2, idx, 8, 1.0, variant=SEQUENTIAL), wrong) and not _same(_cloud(fc, d2, idx, 8, 1.0, variant=SEQUENTIAL), ref)


def test_refuses_a_population_variance(fc, plain_cloud):
    d2, idx, ref = plain_cloud
    wrong = fr.outlier_ref(d2, idx, 8, 1.0, population=True)
    got = _cloud(fc, d2, idx, 8, 1.0, variant=POPULATION)
    assert _same(got, wrong) and not _same(got, ref) and got[1][1] < ref[1][1]


def test_refuses_a_strict_bound(fc):
    x = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])      # every row's nearest neighbour is 1 away: std = 0, thr = mean
    d2, idx = knn_brute(x, 2)
    ref = fr.outlier_ref(d2, idx, 1, 2.0)
    assert list(ref[1]) == [1.0, 0.0, 1.0] and ref[2].all()
    assert _same(_cloud(fc, d2, idx, 1, 2.0), ref)
    got = _cloud(fc, d2, idx, 1, 2.0, variant=STRICT)
    assert _same(got, fr.outlier_ref(d2, idx, 1, 2.0, strict=True)) and not got[2].any() and not _same(got, ref)


def test_refuses_a_self_slot_that_counts(fc, plain_cloud):
    d2, idx, ref = plain_cloud
    got = _cloud(fc, d2, idx, 8, 1.0, variant=KEEP_SELF)
    assert _same(got, fr.outlier_ref(d2, idx, 8, 1.0, skip_self=False)) and not fr.same_bits(got[0], ref[0])
    assert (got[0] < ref[0]).all()                                    # (the zero distance to itself pulls every mean down)


def test_refuses_a_fused_square(fc, plain_cloud):
    d2, idx, ref = plain_cloud
    got = _cloud(fc, d2, idx, 8, 1.0, variant=FUSED)
    assert _same(got, fr.outlier_ref(d2, idx, 8, 1.0, fused=True))
    assert fr.same_bits(got[0], ref[0]) and got[1][0] == ref[1][0]    # the means do not change ...
    assert got[1][1] != ref[1][1] and not _same(got, ref)             # ... the standard deviation does, in its last bits
    assert abs(got[1][1] - ref[1][1]) < 1e-12 * ref[1][1]


# ------------------------------------------------------------------ argument checks: ValueError, no device touched
def test_select_rows_arguments():
    p, mk = torch.zeros(5, 3), torch.ones(5, dtype=torch.bool)
    P, M = torch.zeros(2, 5, 3), torch.ones(2, 5, dtype=torch.bool)
    bad = [
        (p, mk.to(torch.uint8), {}),                                  # mask dtype
        (p, mk.float(), {}),
        (p, [True] * 5, {}),
        (p, torch.ones(2, 5, dtype=torch.bool), {}),                  # form
        (P, mk, {}),
        (P, [mk, mk], {}),
        ([p, p], M, {}),
        (p, torch.ones(4, dtype=torch.bool), {}),                     # length
        (P, torch.ones(2, 4, dtype=torch.bool), {}),
        (P, torch.ones(3, 5, dtype=torch.bool), {}),
        ([p, p], [mk, mk[:4]], {}),
        ([p, p], [mk], {}),
        (p, mk.to("meta"), {}),                                       # device
        (p, mk, {"rows": torch.tensor([3])}),                         # rows with a single cloud
        (P, M, {"rows": torch.tensor([3, 6])}),                       # rows out of range
        (P, M, {"rows": torch.tensor([3.0, 2.0])}),
        ([p, p], [mk, mk], {"rows": torch.tensor([3, 3])}),
        (p.to(torch.float16), mk, {}),                                # points
        (torch.zeros(5), mk, {}),
        (torch.zeros(0, 3), torch.ones(0, dtype=torch.bool), {}),
    ]
    for pts, mask, kw in bad:
        with pytest.raises(ValueError, match="select_rows"):
            select_rows(pts, mask, **kw)


def test_filter_arguments():
    p = torch.zeros(5, 3)
    for kw in ({"k": 0}, {"k": 32}, {"k": 8.0}, {"k": True}, {"std_ratio": -0.5}, {"std_ratio": float("inf")}, {"std_ratio": float("nan")},
               {"std_ratio": True}, {"std_ratio": "2"}, {"std_ratio": torch.tensor(2.0)}, {"method": "brute"}, {"method": None},
               {"rows": torch.tensor([3])}, {"return_mask": 1}, {"return_stats": None}):
        with pytest.raises(ValueError, match="statistical_outlier_removal"):
            statistical_outlier_removal(p, **kw)
    with pytest.raises(ValueError, match="statistical_outlier_removal"):
        statistical_outlier_removal(torch.zeros(5, 2))
    for args, kw in (((0.1, 0), {}), ((0.1, -1), {}), ((0.1, 1.0), {}), ((0.1, True), {}), ((0.1, 2), {"rows": torch.tensor([3])}),
                     ((0.1, 2), {"return_index": 1})):
        with pytest.raises(ValueError, match="radius_outlier_removal"):
            radius_outlier_removal(p, *args, **kw)
    for r in (0.0, -1.0, float("inf"), float("nan"), 1e-50, "1", True):
        with pytest.raises(ValueError, match="radius"):
            radius_outlier_removal(p, r, 2)
    with pytest.raises(ValueError, match="radius_outlier_removal"):
        radius_outlier_removal(torch.zeros(5, 2), 0.1, 2)


# ------------------------------------------------------------------ status codes of the entry points: refused before any launch
NULL, SHAPE, DTYPE, ALIGN = 1, 2, 3, 5
F32, F64 = _lib.F32, _lib.F64
BIG = 1 << 62


def P(addr):
    return ctypes.c_void_p(addr)


OK = P(4096)                                    # aligned for every class; never dereferenced: each call is refused first
OUT = P(8192)


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def entry(fn, good):
    def call(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        assert a != list(good), "a valid call would launch"
        return fn(*a)
    return call


def all_equal(call, positions, value, code, **kw):
    got = {i: call(**dict(kw, **{"a%d" % i: value})) for i in positions}
    assert got == {i: code for i in positions}


def test_select_rows_codes(lib):
    # (dtype, pts, c, mask, rows, N, m, out, rows_out, index, pos, workspace, workspace_bytes, stream)
    need = lib.dicp_select_workspace_bytes(2, 3000)
    assert need == 2 * 256                                            # 2 x 3 tiles: counts and offsets, each rounded up to 256 bytes
    f = entry(lib.dicp_select_rows, [F32, OK, 3, OK, None, 2, 3000, OUT, OK, OK, OK, OK, need, None])
    all_equal(f, (1, 3, 7, 8, 11), None, NULL)
    assert f(a9=None, a10=None, a1=P(4098)) == ALIGN                  # index and pos are optional
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a5=0) == SHAPE and f(a6=0) == SHAPE and f(a2=0) == SHAPE and f(a2=(1 << 16) + 1, a12=BIG) == SHAPE
    assert f(a6=0x7fffffff - 1024, a12=BIG) == SHAPE and f(a6=0x7fffffff - 1025, a12=BIG, a1=P(4098)) == ALIGN
    assert f(a5=1 << 22, a6=1 << 20, a12=BIG) == SHAPE                # more tiles than a grid has blocks
    assert f(a7=OK) == SHAPE                                          # not in place
    assert f(a12=need - 1) == SHAPE and f(a12=need, a1=P(4098)) == ALIGN
    assert f(a11=P(4096 + 128)) == ALIGN
    all_equal(f, (1, 7), P(4096 + 2), ALIGN)
    all_equal(f, (1, 7), P(4096 + 4), ALIGN, a0=F64)
    all_equal(f, (4, 8, 10), P(4096 + 2), ALIGN)
    assert f(a9=P(4096 + 4)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a5=0) == DTYPE and f(a2=0, a1=P(4098)) == SHAPE
    assert lib.dicp_select_workspace_bytes(0, 10) == 0 and lib.dicp_select_workspace_bytes(2, 0) == 0


def test_select_rows_backward_codes(lib):
    # (dtype, grad_out, pos, N, m, c, grad_pts, stream)
    f = entry(lib.dicp_select_rows_backward, [F32, OK, OK, 2, 3000, 3, OUT, None])
    all_equal(f, (1, 2, 6), None, NULL)
    assert f(a0=2) == DTYPE
    assert f(a3=0) == SHAPE and f(a4=0) == SHAPE and f(a5=0) == SHAPE and f(a6=OK) == SHAPE
    all_equal(f, (1, 6), P(4096 + 2), ALIGN)
    all_equal(f, (1, 6), P(4096 + 4), ALIGN, a0=F64)
    assert f(a2=P(4096 + 2)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a3=0) == DTYPE and f(a5=0, a1=P(4098)) == SHAPE


def test_outlier_stats_codes(lib):
    # (dtype, d2, idx, rows, N, m, k, std_ratio, mean_distance, stats, mask, workspace, workspace_bytes, stream)
    need = lib.dicp_outlier_workspace_bytes(2, 3000)
    assert need > 2 * 3000 * 9 and need % 256 == 0
    f = entry(lib.dicp_outlier_stats, [F32, OK, OK, None, 2, 3000, 16, 2.0, OK, OK, OK, OK, need, None])
    all_equal(f, (1, 2, 8, 9, 10, 11), None, NULL)
    assert f(a0=2) == DTYPE
    assert f(a4=0) == SHAPE and f(a5=0) == SHAPE and f(a6=0) == SHAPE and f(a6=32) == SHAPE
    assert f(a6=31, a1=P(4098)) == ALIGN and f(a6=1, a1=P(4098)) == ALIGN
    for r in (-1.0, float("inf"), float("nan")):
        assert f(a7=r) == SHAPE
    assert f(a7=0.0, a1=P(4098)) == ALIGN
    assert f(a12=need - 1) == SHAPE and f(a12=need, a1=P(4098)) == ALIGN
    assert f(a11=P(4096 + 128)) == ALIGN
    assert f(a1=P(4096 + 2)) == ALIGN and f(a1=P(4096 + 4), a0=F64, a12=BIG) == ALIGN
    all_equal(f, (2, 8, 9), P(4096 + 4), ALIGN)
    assert f(a3=P(4096 + 2)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a4=0) == DTYPE and f(a6=0, a1=P(4098)) == SHAPE
    assert lib.dicp_outlier_workspace_bytes(0, 10) == 0 and lib.dicp_outlier_workspace_bytes(2, 0) == 0
