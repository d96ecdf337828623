"""knn_points / chamfer_distance on the MI355X where the neighbour lists leave the kernels' LDS windows (csrc/knn_points.hip: the forward
walk's global reads, the backward's global atomics and its capped window), on the layouts of tests/walk_layouts.py.

Every case first asserts, with the numpy window model on the brute force's lists, that its input reaches the code it is meant for (the
conditions of walk_layouts.check_knn_conditions; tests/test_walk_layouts.py holds the same conditions without a GPU).  The forward is held to
the brute force index for index and bit for bit, on every query.  The gradients are held, value by value, to float64 terms formed from the
kernel's lists, within bounds derived from k, the in-degree D, the unit roundoff u_T and sum |t| (walk_layouts.knn_grad_terms): no tolerance
here is a literal.  In float64 the y-gradient's bound is ~1e-13 of the sum of its terms' magnitudes, nine orders below any single term, so one
lost, doubled or misplaced contribution fails.  In float32 on dense_queries (in-degree ~3000) the bound (D + 2) 2^-24 sum |t| is about the
size of one term: that layout's float32 run still checks the pile-up's rounding, and its float64 run is the one that counts contributions."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.knn import chamfer_distance, knn_points

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import walk_layouts as wl  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    """-> (X, Y in the dtype, k, the brute force's d2 and idx, the window model on those lists), the layout's conditions asserted"""
    x, y, k = wl.knn_layout(name, dtype)
    dt = wl.np_dtype(dtype)
    X, Y = x.astype(dt), y.astype(dt)
    d2o, io = wl.knn_oracle(X, Y, k)
    w = wl.knn_windows(X, Y, k, dtype, io)
    print("%s %s: fwd outside %.3f, bwd outside %.3f, capped bwd windows %d of %d, max in-degree %d"
          % (name, dt.name, w.share("fwd"), w.share("bwd"), w.capped_bwd, w.blocks, w.indegree.max()))
    wl.check_knn_conditions(name, dtype, w)
    return X, Y, k, d2o, io, w


def _g(shape, dtype, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(wl.np_dtype(dtype))


def _run(X, Y, k, g, masked=True, **kw):
    """one forward + backward on the GPU -> d2, idx, x.grad, y.grad as numpy"""
    x = torch.from_numpy(X).cuda().requires_grad_(True)
    y = torch.from_numpy(Y).cuda().requires_grad_(True)
    d2, idx = knn_points(x, y, k=k, **kw)
    gt = torch.from_numpy(g).cuda()
    if masked:
        gt = torch.where(idx >= 0, gt, torch.zeros_like(gt))
    torch.autograd.backward(d2, gt)
    return d2.detach().cpu().numpy(), idx.cpu().numpy(), x.grad.cpu().numpy(), y.grad.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", wl.KNN_LAYOUTS)
def test_forward_exact(name, dtype):
    X, Y, k, d2o, io, w = _case(name, dtype)
    assert X.shape[0] * Y.shape[0] <= 5e8                   # every query is compared
    d2, idx = knn_points(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), k=k)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    bad = np.flatnonzero((idx != io).any(1))
    assert bad.size == 0, "%d queries differ (%d of them with entries outside the forward window), first %d: %s vs %s" % (
        bad.size, int(w.fwd_outside[bad].any(1).sum()), bad[0], idx[bad[0]], io[bad[0]])
    assert _same_bits(d2, d2o)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", wl.KNN_LAYOUTS)
def test_gradients_within_derived_bounds(name, dtype):
    X, Y, k, d2o, io, w = _case(name, dtype)
    g = _g(io.shape, dtype, 7)
    d2, idx, gx, gy = _run(X, Y, k, g)
    assert np.array_equal(idx, io)                          # (test_forward_exact; the terms below are formed on these lists)
    rx, ry = wl.knn_grad_check(X, Y, idx, g, gx, gy, dtype, name)
    print("%s %s: worst error / bound: x-gradient %.3f, y-gradient %.3f" % (name, wl.np_dtype(dtype).name, rx, ry))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batch_of_hard_layouts_against_single_calls(dtype):
    """wall, sparse_queries, two_clusters, edge_m-1 and a cloud without queries in one padded call (N = 5), the padding filled with points
    that would be neighbours if a row count were ignored.  A wrong cloud offset on the out-of-window paths (ybase) shows here and nowhere
    else.  Every window of the first three clouds ends at its cap; edge_m-1 is the cloud whose row count (W - 1 of 60000 stored targets) ends
    the staged window: whi = min(span[1] + H, mb) = mb."""
    dt = wl.np_dtype(dtype)
    names = ("wall", "sparse_queries", "two_clusters", "edge_m-1")
    cases = [_case(nm, dtype) for nm in names]
    N, n, m, k = 5, 20000, 60000, 8                         # (edge_m's own k is 4: its lists are taken from its single call at k = 8 below)
    xr, yr = [c[0].shape[0] for c in cases] + [0], [c[1].shape[0] for c in cases] + [1000]
    assert all(c[2] == k for c in cases[:3]) and max(xr) == n and max(yr) == m
    X = np.stack([wl.cube(n, 100 + b) for b in range(N)]).astype(dt)
    Y = np.stack([wl.cube(m, 200 + b) for b in range(N)]).astype(dt)
    X[0], Y[0] = wl.wall(n, 100).astype(dt), wl.wall(m, 200).astype(dt)     # (the wall's padding lies in the wall)
    for b, c in enumerate(cases):
        X[b, :xr[b]], Y[b, :yr[b]] = c[0], c[1]
    g = _g((N, n, k), dtype, 11)
    rows = dict(x_rows=torch.tensor(xr), y_rows=torch.tensor(yr))
    d2, idx, gx, gy = _run(X, Y, k, g, **rows)
    for b in range(N):
        assert np.all(idx[b, xr[b]:] == -1) and np.all(np.isposinf(d2[b, xr[b]:]))
        assert np.all(gx[b, xr[b]:] == 0) and np.all(gy[b, yr[b]:] == 0)
        if xr[b] == 0:
            assert np.all(gy[b] == 0)
            continue
        Xb, Yb = X[b, :xr[b]], Y[b, :yr[b]]
        d1, i1, gx1, gy1 = _run(Xb, Yb, k, g[b, :xr[b]])
        if names[b] == "edge_m-1":
            # the row count is the smallest of the three terms of whi, on the values: span[1] + H > mb and mb <= wlo + W in the one block,
            # while 57000 stored rows beyond it would be nearer than most of the lists' rows
            d2o, io = wl.knn_oracle(Xb, Yb, k)
            assert np.array_equal(i1, io) and _same_bits(d1, d2o)
            w = wl.knn_windows(Xb, Yb, k, dtype, io)
            assert yr[b] == wl.win_rows(dtype) - 1 < m and w.blocks == 1 and w.rows_bind_fwd == 1 and w.capped_fwd == 0
        else:
            assert np.array_equal(i1, cases[b][4])          # (the single call is the one test_forward_exact holds to the brute force)
        assert np.array_equal(idx[b, :xr[b]], i1), "cloud %d (%s)" % (b, names[b])
        assert _same_bits(d2[b, :xr[b]], d1) and _same_bits(gx[b, :xr[b]], gx1), "cloud %d (%s)" % (b, names[b])
        wl.knn_grad_check(Xb, Yb, i1, g[b, :xr[b]], gx[b, :xr[b]], gy[b, :yr[b]], dtype, "batch cloud %d (%s)" % (b, names[b]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_six_columns_on_sparse_queries(dtype):
    """pt2pl rows (6 columns) on a layout that leaves the window: the same lists and xyz gradients within the same bounds, exactly 0 beyond"""
    X, Y, k, d2o, io, w = _case("sparse_queries", dtype)
    dt = wl.np_dtype(dtype)
    X6 = np.concatenate([X, wl.cube(X.shape[0], 31).astype(dt)], 1)
    Y6 = np.concatenate([Y, wl.cube(Y.shape[0], 32).astype(dt)], 1)
    g = _g(io.shape, dtype, 33)
    d2, idx, gx, gy = _run(X6, Y6, k, g)
    assert np.array_equal(idx, io) and _same_bits(d2, d2o)
    assert gx.shape == X6.shape and gy.shape == Y6.shape and np.all(gx[:, 3:] == 0) and np.all(gy[:, 3:] == 0)
    wl.knn_grad_check(X, Y, idx, g, gx[:, :3], gy[:, :3], dtype, "six columns")


@pytest.mark.parametrize("pair", ["sparse_dense", "wall"])
def test_chamfer_against_float64_oracle(pair):
    """One call of chamfer_distance(sparse, dense) searches in the 0.94-outside direction and in the high-in-degree direction."""
    X, Y, _, _, io8, _ = _case("sparse_queries" if pair == "sparse_dense" else "wall", torch.float64)
    n, m = X.shape[0], Y.shape[0]
    xd = torch.from_numpy(X).cuda().requires_grad_(True)
    yd = torch.from_numpy(Y).cuda().requires_grad_(True)
    val = chamfer_distance(xd, yd)
    val.backward()
    xo = torch.from_numpy(X).requires_grad_(True)
    yo = torch.from_numpy(Y).requires_grad_(True)
    ref = wl.chamfer_oracle([xo], [yo], chunk_elems=4_000_000)[0]
    ref.backward()
    torch.testing.assert_close(val.cpu(), ref.detach(), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(xd.grad.cpu(), xo.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(yd.grad.cpu(), yo.grad, rtol=1e-10, atol=1e-12)
    # value by value within the derived bounds: each cloud is the query side of one k = 1 search (upstream gradient 1 / its row count, the
    # x-gradient's rule) and the target side of the other (the y-gradient's rule); autograd adds the two with one more rounding
    _, ixy = knn_points(xd.detach(), yd.detach(), k=1)
    _, iyx = knn_points(yd.detach(), xd.detach(), k=1)
    ixy, iyx = ixy.cpu().numpy(), iyx.cpu().numpy()
    assert np.array_equal(ixy[:, 0], io8[:, 0])             # (the nearest row of the k = 8 brute force)
    assert wl.knn_windows(X, Y, 1, np.float64, ixy).share("bwd") >= 0.5
    if pair == "sparse_dense":                              # the other direction: 200 nearest-neighbour entries per row of x on average
        assert wl.knn_windows(Y, X, 1, np.float64, iyx).indegree.max() >= wl.BLOCK
    gxy, gyx = np.full((n, 1), np.float64(1.0) / n), np.full((m, 1), np.float64(1.0) / m)
    Sx1, Bx1, Sy1, By1, _ = wl.knn_grad_terms(X, Y, ixy, gxy, np.float64)
    Sx2, Bx2, Sy2, By2, _ = wl.knn_grad_terms(Y, X, iyx, gyx, np.float64)
    u = wl.U[np.dtype(np.float64)]
    wl.assert_within(xd.grad.cpu().numpy(), Sx1 + Sy2, Bx1 + By2 + u * (np.abs(Sx1) + np.abs(Sy2)), "chamfer x-gradient")
    wl.assert_within(yd.grad.cpu().numpy(), Sy1 + Sx2, By1 + Bx2 + u * (np.abs(Sy1) + np.abs(Sx2)), "chamfer y-gradient")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_forward_and_x_gradient_bit_reproducible_on_the_wall(dtype):
    X, Y, k, _, _, _ = _case("wall", dtype)
    g = _g((X.shape[0], k), dtype, 13)
    a, b = _run(X, Y, k, g), _run(X, Y, k, g)
    assert _same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and _same_bits(a[2], b[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_missing_neighbours_ignore_their_upstream_gradient(dtype):
    """k = 32 against 5 targets and a NaN query: idx = -1 in most slots, a finite upstream gradient in every one of them"""
    dt = wl.np_dtype(dtype)
    X, Y = wl.cube(300, 21).astype(dt), wl.cube(5, 22).astype(dt)
    X[7, 0] = np.nan
    g = _g((300, 32), dtype, 23)
    d2, idx, gx, gy = _run(X, Y, 32, g, masked=False)
    assert np.all(idx[7] == -1) and np.all(idx[:, 5:] == -1) and np.all(idx[np.arange(300) != 7, :5] >= 0)
    d2m, idxm, gxm, gym = _run(X, Y, 32, g, masked=True)
    assert np.array_equal(idx, idxm) and _same_bits(gx, gxm) and np.all(gx[7] == 0)
    assert np.all(np.isfinite(gx)) and np.all(np.isfinite(gy))
    Xf = np.where(np.isnan(X), dt.type(0), X)                # (row 7 has no kept entry: its coordinates enter no term)
    wl.knn_grad_check(Xf, Y, idx, g, gx, gy, dtype, "unmasked")
    wl.knn_grad_check(Xf, Y, idx, g, gxm, gym, dtype, "masked")
