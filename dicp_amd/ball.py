"""Differentiable fixed-radius neighbours between two clouds, on a sorted cell grid.

Exact results on the GPU (libdicp_hip.so: dicp_ball_grid_build / dicp_ball_query / dicp_ball_query_backward), without the (n, m) distance
matrix and without a dense table of cells:

    from dicp_amd.ball import ball_query
    d2, idx = ball_query(x, y, radius=0.2, k=16)                          # the nearest k rows of y inside the radius, (..., n, k)
    d2, idx, counts = ball_query(x, y, 0.2, k=16, return_counts=True)     # and how many rows the ball holds, never capped by k
"""
import math

import torch

from . import _clouds
from ._clouds import ROW, K_MIN, K_MAX
from ._grid import CellGrid, _backward, _forward    # (CellGrid: also for the callers that import it from here)
from ._ops import _DT


class _BallQuery(torch.autograd.Function):
    """(x (N,n,c), y (N,m,c)) -> (d2 (N,n,k), idx (N,n,k) int64, counts (N,n) int32) on y's grid: one library call per direction."""

    @staticmethod
    def forward(ctx, x, y, grid, xkeys, xperm, k, visited, det=False):
        return _forward(ctx, "dicp_ball_query", x, y, grid, xkeys, xperm, k, True, (visited,), det)

    @staticmethod
    def backward(ctx, g_d2, _g_idx, _g_counts):
        return _backward(ctx, g_d2, 8)


def _err(msg):
    raise ValueError(msg)


def _check_radius(radius):
    """-> a Python float (checked: finite and > 0) or a 0-d device tensor (not read back: see ball_query)"""
    if isinstance(radius, torch.Tensor):
        if radius.dim() != 0 or not radius.dtype.is_floating_point:
            _err("ball_query: radius must be a float or a 0-d floating-point tensor, got a tensor of shape %s and dtype %s"
                 % (tuple(radius.shape), radius.dtype))
        if radius.is_cuda:
            return radius
        radius = float(radius)
    if isinstance(radius, bool) or not isinstance(radius, (int, float)):
        _err("ball_query: radius must be a float or a 0-d tensor, got %s" % type(radius).__name__)
    if isinstance(radius, int) and abs(radius) > 2 ** 1023:
        _err("ball_query: radius must be finite and > 0, got %r" % (radius,))
    radius = float(radius)
    if not (math.isfinite(radius) and radius > 0.0):
        _err("ball_query: radius must be finite and > 0, got %r" % (radius,))
    return radius


def ball_query(x, y, radius, k=16, x_rows=None, y_rows=None, return_counts=False, _visited=None, deterministic=False):
    """The rows of y within `radius` of every row of x: the nearest k of them, and optionally how many there are, exactly.

    x, y, x_rows, y_rows: as knn_points -- one cloud each (n, c) and (m, c); a padded batch each (N, n, c) and (N, m, c) with optional
        integer row counts (N,); or two lists of N clouds.  Both in the same form, dtype (float32 or float64) and device; columns 0:3 are
        used.  CPU tensors are computed on the GPU and returned on the CPU.
    radius: one radius for the whole call, a Python float or a 0-d tensor, finite and > 0.  It is converted to the points' dtype T first,
        then r2 = radius_T * radius_T, rounded in T.  (A 0-d tensor that lives on the device is not read back, so it cannot be checked
        here: a value that is not a finite number > 0 in T gives every query count 0.)
    k: an int in [1, 32].
    deterministic: a bool (anything else is a ValueError before any device work); see "Gradients".

    Definition: d2(i, j) is knn_points' own, (xx + yy) + zz with dx = y_j.x - x_i.x, xx = dx * dx (and so on) as separate roundings in T.
    The candidates of query i of cloud b are the rows j < y_rows[b] whose d2 is finite and d2 <= r2 -- the bound is inclusive.
    counts[b, i] is their number, exact and never capped by k.  d2 / idx hold the first min(k, count) candidates in (d2, index) order;
    slots beyond that hold d2 = +inf and idx = -1, and so do query rows at or past x_rows[b] and queries with a non-finite coordinate
    (their count is 0).  So ball_query(x, y, r, k) equals knn_points(x, y, k) with every entry whose d2 > r2 replaced by (+inf, -1),
    bit for bit.  This is knn_points' convention and NOT PyTorch3D's ball_query, which returns the first k rows in index order, pads d2
    with 0 and compares strictly (d2 < r2).

    Returns (d2, idx) or (d2, idx, counts): (n, k) for single clouds, (N, n, k) for a batch, lists of (n_b, k) for lists; d2 in x's dtype,
    idx int64; counts int32 of shape (n,) / (N, n) / a list of (n_b,).

    Gradients flow from d2 to x[..., :3] (sum_j 2 g_ij (x_i - y_idx)) and y[..., :3] (-sum 2 g_ij (x_i - y_l) over the entries with idx = l);
    other columns, pad rows and empty slots get zero whatever cotangent arrives there (NaN and inf included), and neither the choice of
    neighbours nor counts carries any.  The forward and the x-gradient (written once per row) are bit-reproducible.  The y-gradient is
    by default added with float atomics, as knn_points' is, and its last bits can differ from run to run.  With deterministic=True it is
    summed as knn_points describes -- per row of y over the row's list in the inverted index of idx, in chunks of 64 list positions,
    stored once -- and is bit-reproducible too; the forward and the x-gradient are the default call's, bit for bit.

    y is sorted into a cell grid (CellGrid: the cell edge is the search half-width, a little above the radius, enlarged per cloud on the
    device where extent / radius would not fit a 64-bit key), the queries are processed in the order of its cells, and every query scans
    only the cells its ball can touch.  Nothing is read back from the device: with device tensors and device (or no) row counts a call
    is kernels only.
    """
    _clouds._check_k(k, "ball_query", K_MIN, K_MAX)
    _clouds._check_deterministic(deterministic, "ball_query")
    radius = _check_radius(radius)
    first = x[0] if isinstance(x, (list, tuple)) and x else x
    if isinstance(radius, float) and isinstance(first, torch.Tensor) and first.dtype in _DT:
        r_t = float(torch.tensor(radius, dtype=first.dtype))
        if not (math.isfinite(r_t) and r_t > 0.0):
            _err("ball_query: radius must be finite and > 0 in %s, got %r" % (first.dtype, radius))
    form, on_cpu, lens, n, _, xb, yb, rx, ry = _clouds.pair(x, y, x_rows, y_rows, "ball_query")
    if isinstance(radius, torch.Tensor):
        r_d = radius.detach().to(device=xb.device, dtype=xb.dtype).reshape(1)
    else:
        r_d = torch.full((1,), radius, dtype=xb.dtype, device=xb.device)         # (filled on the device, rounded to T: no copy)
    grid = CellGrid(yb.detach(), ry, r_d)
    xkeys, xperm = grid.order(xb.detach(), rx)
    d2, idx, counts = _BallQuery.apply(xb, yb, grid, xkeys, xperm, k, _visited, deterministic)
    return _clouds.restore(form, on_cpu, n, lens, [(ROW, d2), (ROW, idx)] + ([(ROW, counts)] if return_counts else []))
