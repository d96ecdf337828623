"""CPU checks of dicp_amd.knn that need no GPU.

``dicp_amd/csrc/dicp_topk.h`` -- the lower bound and the two-cursor walk the HIP kernels run -- is compiled with g++ through
tests/hostcheck/knn_check.cpp and held index for index, and d2 bit for bit, to a numpy brute force that computes d2 with the same statements,
on inputs that are hard for a walk over one sorted axis; the argument checks of knn_points / chamfer_distance run before any device work.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.knn import chamfer_distance, knn_points

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostbuild  # noqa: E402


@pytest.fixture(scope="module")
def kc():
    lib = hostbuild.build("knn_check.cpp", "knn_check")
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    for name in ("kc_knn_f32", "kc_knn_f64"):
        fn = getattr(lib, name)
        fn.argtypes = [vp, i32, vp, vp, vp, i32, i32, vp, vp, vp]
        fn.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _walk(kc, X, Y, k):
    """the header's search: Y sorted by x (stable, NaN last, as dicp_sweep_sort), every query of X walked -> (d2, idx, walked)"""
    X = np.ascontiguousarray(X)
    order = np.argsort(Y[:, 0], kind="stable").astype(np.int32)
    Ys = np.ascontiguousarray(Y[order])
    keys = np.ascontiguousarray(Ys[:, 0])
    n, m = X.shape[0], Y.shape[0]
    d2 = np.zeros((n, k), dtype=X.dtype)
    idx = np.zeros((n, k), dtype=np.int64)
    walked = np.zeros(n, dtype=np.uint32)
    fn = kc.kc_knn_f32 if X.dtype == np.float32 else kc.kc_knn_f64
    fn(_p(X), n, _p(Ys), _p(keys), _p(order), m, k, _p(d2), _p(idx), _p(walked))
    return d2, idx, walked


def _oracle(X, Y, k):
    """numpy brute force with the definition's statements, in the inputs' dtype: the first min(k, #finite) rows in (d2, index) order"""
    n, m = X.shape[0], Y.shape[0]
    d2o = np.full((n, k), np.inf, dtype=X.dtype)
    io = np.full((n, k), -1, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = Y[None, :, 0] - X[:, None, 0]
        dy = Y[None, :, 1] - X[:, None, 1]
        dz = Y[None, :, 2] - X[:, None, 2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        d2 = (xx + yy) + zz
    for i in range(n):
        cand = np.flatnonzero(np.isfinite(d2[i]))
        order = np.lexsort((cand, d2[i, cand]))[:k]
        io[i, :len(order)] = cand[order]
        d2o[i, :len(order)] = d2[i, cand[order]]
    return d2o, io


def _same(kc, X, Y, k):
    d2, idx, _ = _walk(kc, X, Y, k)
    d2o, io = _oracle(X, Y, k)
    bad = np.flatnonzero((idx != io).any(1))
    assert bad.size == 0, "%d queries differ, first %d: %s vs %s" % (bad.size, bad[0], idx[bad[0]], io[bad[0]])
    assert np.array_equal(d2.view(np.uint8), d2o.view(np.uint8))
    return d2, idx


DTYPES = (np.float32, np.float64)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", (1, 2, 5, 8, 16, 17, 32))
def test_walk_random(kc, dt, k):
    rng = np.random.default_rng(k)
    X = rng.standard_normal((300, 3)).astype(dt)
    Y = rng.standard_normal((257, 3)).astype(dt)
    _same(kc, X, Y, k)


@pytest.mark.parametrize("dt", DTYPES)
def test_walk_integer_grid_ties_and_duplicates(kc, dt):
    rng = np.random.default_rng(1)
    Y = rng.integers(-3, 4, (400, 3)).astype(dt)
    Y[200:260] = Y[:60]                                 # duplicate rows: equal d2, index order decides
    X = rng.integers(-4, 5, (300, 3)).astype(dt) * dt(0.5)
    for k in (1, 3, 8, 32):
        _same(kc, X, Y, k)


@pytest.mark.parametrize("dt", DTYPES)
def test_walk_wall_perpendicular_to_x(kc, dt):
    rng = np.random.default_rng(2)
    Y = np.concatenate([np.zeros((500, 1)), rng.uniform(-1, 1, (500, 2))], 1).astype(dt)     # every row on x = 0
    Y[::7, 0] = dt(1.0)
    X = np.concatenate([rng.uniform(-0.1, 0.1, (200, 1)), rng.uniform(-1, 1, (200, 2))], 1).astype(dt)
    X[:50, 0] = 0                                       # queries on the wall itself
    for k in (1, 4, 16):
        _same(kc, X, Y, k)


@pytest.mark.parametrize("dt", DTYPES)
def test_walk_queries_outside_the_x_range(kc, dt):
    rng = np.random.default_rng(3)
    Y = rng.uniform(0, 1, (300, 3)).astype(dt)
    X = rng.uniform(0, 1, (100, 3)).astype(dt)
    X[:50, 0] += dt(100.0)
    X[50:, 0] -= dt(100.0)
    for k in (1, 8, 32):
        _, _, walked = _walk(kc, X, Y, k)
        _same(kc, X, Y, k)
        assert walked.max() <= 300


@pytest.mark.parametrize("dt", DTYPES)
def test_walk_nan_and_huge_rows(kc, dt):
    rng = np.random.default_rng(4)
    Y = rng.standard_normal((200, 3)).astype(dt)
    Y[5, 0] = np.nan                                    # NaN in the sorted key: sorts last
    Y[17, 1] = np.nan
    Y[40:45] = dt(np.finfo(dt).max / 2)                 # d2 overflows to +inf: not candidates
    Y[60, 2] = np.inf
    X = rng.standard_normal((120, 3)).astype(dt)
    X[3, 0] = np.nan                                    # queries with a non-finite coordinate: no neighbours, the walk still ends
    X[4, 2] = np.nan
    X[5, 0] = np.inf
    X[6, 1] = -np.inf
    X[7] = dt(np.finfo(dt).max / 2)
    for k in (1, 4, 32):
        d2, idx = _same(kc, X, Y, k)
        assert np.all(idx[3:7] == -1) and np.all(np.isinf(d2[3:7]))


@pytest.mark.parametrize("dt", DTYPES)
def test_walk_k_above_m(kc, dt):
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((5, 3)).astype(dt)
    X = rng.standard_normal((40, 3)).astype(dt)
    for k in (6, 17, 32):
        d2, idx = _same(kc, X, Y, k)
        assert np.all(idx[:, 5:] == -1) and np.all(d2[:, 5:] == np.inf)
        assert np.all(np.sort(idx[:, :5], 1) == np.arange(5))


@pytest.mark.parametrize("dt", DTYPES)
def test_walk_empty_target(kc, dt):
    X = np.zeros((3, 3), dtype=dt)
    d2, idx, walked = _walk(kc, X, np.zeros((0, 3), dtype=dt), 4)
    assert np.all(idx == -1) and np.all(d2 == np.inf) and np.all(walked == 0)


# ---------------------------------------------------------------- argument checks (before any device work)

def _raises(fn, *a, **kw):
    with pytest.raises(ValueError):
        fn(*a, **kw)


def test_knn_points_rejects_bad_arguments():
    x, y = torch.rand(5, 3), torch.rand(4, 3)
    for k in (0, 33, -1, 1.0, True, "8", None):
        _raises(knn_points, x, y, k=k)
    _raises(knn_points, x.double(), y, k=1)                           # mixed dtypes
    _raises(knn_points, x.half(), y.half(), k=1)                      # unsupported dtype
    _raises(knn_points, x.to(torch.int64), y.to(torch.int64), k=1)
    _raises(knn_points, torch.rand(5, 2), torch.rand(4, 2), k=1)      # fewer than 3 columns
    _raises(knn_points, torch.rand(2, 2, 5, 3), torch.rand(2, 2, 4, 3), k=1)
    _raises(knn_points, x, torch.rand(1, 4, 3), k=1)                  # mixed forms
    _raises(knn_points, [x], y, k=1)
    _raises(knn_points, torch.rand(2, 5, 3), torch.rand(3, 4, 3), k=1)    # batch sizes differ
    _raises(knn_points, [x, x], [y], k=1)
    _raises(knn_points, [], [], k=1)
    _raises(knn_points, [x, x.double()], [y, y], k=1)
    _raises(knn_points, [x, torch.rand(5, 6)], [y, y], k=1)
    _raises(knn_points, x, y, k=1, x_rows=torch.tensor([5]))          # row counts need a padded batch
    _raises(knn_points, [x], [y], k=1, y_rows=torch.tensor([4]))
    xb, yb = torch.rand(2, 5, 3), torch.rand(2, 4, 3)
    _raises(knn_points, xb, yb, k=1, x_rows=torch.tensor([1, 6]))     # out of range
    _raises(knn_points, xb, yb, k=1, y_rows=torch.tensor([-1, 2]))
    _raises(knn_points, xb, yb, k=1, y_rows=torch.tensor([1, 2, 3]))  # wrong count
    _raises(knn_points, xb, yb, k=1, y_rows=torch.tensor([1.0, 2.0]))
    _raises(knn_points, xb, yb, k=1, y_rows=torch.tensor([True, False]))
    _raises(knn_points, "x", y, k=1)


def test_chamfer_rejects_bad_arguments():
    x, y = torch.rand(5, 3), torch.rand(4, 3)
    for r in ("max", "", None, 1, "MEAN"):
        _raises(chamfer_distance, x, y, reduction=r)
    _raises(chamfer_distance, x, y.double())
    _raises(chamfer_distance, x, torch.rand(1, 4, 3))
    _raises(chamfer_distance, torch.rand(2, 5, 3), torch.rand(2, 4, 3), x_rows=torch.tensor([0, 9]))
    _raises(chamfer_distance, torch.rand(5, 2), torch.rand(4, 2))
