"""Differentiable fixed-radius neighbours between two clouds, on a sorted cell grid.

Exact results on the GPU (libdicp_hip.so: dicp_ball_grid_build / dicp_ball_query / dicp_ball_query_backward), without the (n, m) distance
matrix and without a dense table of cells:

    from dicp_amd.ball import ball_query
    d2, idx = ball_query(x, y, radius=0.2, k=16)                          # the nearest k rows of y inside the radius, (..., n, k)
    d2, idx, counts = ball_query(x, y, 0.2, k=16, return_counts=True)     # and how many rows the ball holds, never capped by k
"""
import math

import torch

from . import _clouds, _lib
from ._clouds import ROW
from ._ops import _DT, _p, _stream, _on
from .knn import K_MIN, K_MAX


class CellGrid:
    """The cell grid of every cloud of a batch (dicp_ball_grid_build): the rows sorted by a 64-bit cell key.

    pts (N,m,c) on the device, rows (N,) int32 or None, radius a (1,) device tensor of pts' dtype.  keys (N,P) int64 holding the unsigned
    keys, perm (N,P) int32, rows4 (N,P,4) the live rows packed in sorted order, plans the per-cloud origin / cell edges / key widths /
    live-row count, all chosen on the device.  P = dicp_ball_grid_slots(m); memory is O(m) per cloud whatever extent / radius is.
    """

    def __init__(self, pts, rows, radius):
        self._build(pts, rows, lambda lib, dt, N, m, c: lib.dicp_ball_grid_build(
            dt, _p(pts), c, _p(rows), N, m, _p(radius), None, _p(self.plans), _p(self.keys), _p(self.perm), _p(self.rows4), _stream()),
            "dicp_ball_grid_build")

    @classmethod
    def by_density(cls, pts, rows):
        """The grid without a radius (dicp_knn_grid_build), for the k-NN search: the cell edge is chosen per cloud on the device from the
        number and the bounds of its live rows, about two rows per cell of the bounding box (csrc/dicp_gridknn.h)."""
        self = cls.__new__(cls)
        self._build(pts, rows, lambda lib, dt, N, m, c: lib.dicp_knn_grid_build(
            dt, _p(pts), c, _p(rows), N, m, _p(self.plans), _p(self.keys), _p(self.perm), _p(self.rows4), _stream()), "dicp_knn_grid_build")
        return self

    def _build(self, pts, rows, call, what):
        N, m, c = pts.shape
        lib = _lib.load()
        dev = pts.device
        self.shape = (N, m, c)
        self.slots = P = lib.dicp_ball_grid_slots(m)
        self.plans = torch.empty((N, lib.dicp_ball_plan_bytes()), dtype=torch.uint8, device=dev)
        self.keys = torch.empty((N, P), dtype=torch.int64, device=dev)
        self.perm = torch.empty((N, P), dtype=torch.int32, device=dev)
        self.rows4 = torch.empty((N, P, 4), dtype=pts.dtype, device=dev)
        with _on(dev):
            _lib.check(call(lib, _DT[pts.dtype], N, m, c), what)

    def order(self, x, x_rows):
        """-> (keys (N,Pn) int64, perm (N,Pn) int32): the rows of x (N,n,c) in the order of this grid's cells"""
        N, n, c = x.shape
        lib = _lib.load()
        Pn = lib.dicp_ball_grid_slots(n)
        keys = torch.empty((N, Pn), dtype=torch.int64, device=x.device)
        perm = torch.empty((N, Pn), dtype=torch.int32, device=x.device)
        with _on(x.device):
            _lib.check(lib.dicp_ball_grid_build(_DT[x.dtype], _p(x), c, _p(x_rows), N, n, None, _p(self.plans), None, _p(keys), _p(perm), None,
                                                _stream()), "dicp_ball_grid_build")
        return keys, perm


class _BallQuery(torch.autograd.Function):
    """(x (N,n,c), y (N,m,c)) -> (d2 (N,n,k), idx (N,n,k) int64, counts (N,n) int32) on y's grid: one library call per direction."""

    @staticmethod
    def forward(ctx, x, y, grid, xkeys, xperm, k, visited):
        N, n, cx = x.shape
        m, cy = y.shape[1], y.shape[2]
        dt = _DT[x.dtype]
        lib = _lib.load()
        dev = x.device
        ws_bytes = lib.dicp_ball_query_workspace_bytes(dt, N, n, k)
        d2 = torch.empty((N, n, k), dtype=x.dtype, device=dev)
        idx = torch.empty((N, n, k), dtype=torch.int64, device=dev)
        counts = torch.empty((N, n), dtype=torch.int32, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with _on(dev):
            _lib.check(lib.dicp_ball_query(dt, _p(x), cx, n, _p(xkeys), _p(xperm), _p(grid.plans), _p(grid.keys), _p(grid.perm), _p(grid.rows4),
                                           m, N, k, _p(d2), _p(idx), _p(counts), _p(ws), ws_bytes, _p(visited), _stream()), "dicp_ball_query")
        ctx.save_for_backward(x)
        ctx.grid, ctx.ws, ctx.k, ctx.shape = grid, ws, k, (N, n, cx, m, cy)
        ctx.mark_non_differentiable(idx, counts)
        ctx.set_materialize_grads(False)
        return d2, idx, counts

    @staticmethod
    def backward(ctx, g_d2, _g_idx, _g_counts):
        return _backward(ctx, g_d2, 7)


def _backward(ctx, g_d2, n_inputs):
    """dicp_ball_query_backward from what a forward on a CellGrid saved: the gradients of x and y, None for the other inputs"""
    nothing = (None,) * n_inputs
    want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if g_d2 is None or not (want_x or want_y):
        return nothing
    x, = ctx.saved_tensors
    N, n, cx, m, cy = ctx.shape
    grid = ctx.grid
    dtype, dev = g_d2.dtype, g_d2.device
    gx = torch.empty((N, n, cx), dtype=dtype, device=dev) if want_x else None
    gy = torch.empty((N, m, cy), dtype=dtype, device=dev) if want_y else None
    g_d2 = g_d2.contiguous()
    with _on(dev):
        _lib.check(_lib.load().dicp_ball_query_backward(_DT[dtype], _p(g_d2), _p(x), cx, n, _p(grid.rows4), _p(grid.perm), m, cy, N, ctx.k,
                                                        _p(ctx.ws), _p(gx), _p(gy), _stream()), "dicp_ball_query_backward")
    return (gx, gy) + nothing[2:]


class _GridKnn(torch.autograd.Function):
    """(x (N,n,c), y (N,m,c)) -> (d2 (N,n,k), idx (N,n,k) int64): the k nearest rows on y's density grid (dicp_knn_grid_query); the
    backward is ball_query's."""

    @staticmethod
    def forward(ctx, x, y, grid, xkeys, xperm, k, visited, passes):
        N, n, cx = x.shape
        m, cy = y.shape[1], y.shape[2]
        dt = _DT[x.dtype]
        lib = _lib.load()
        dev = x.device
        ws_bytes = lib.dicp_ball_query_workspace_bytes(dt, N, n, k)
        d2 = torch.empty((N, n, k), dtype=x.dtype, device=dev)
        idx = torch.empty((N, n, k), dtype=torch.int64, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with _on(dev):
            _lib.check(lib.dicp_knn_grid_query(dt, _p(x), cx, n, _p(xkeys), _p(xperm), _p(grid.plans), _p(grid.keys), _p(grid.perm), _p(grid.rows4),
                                               m, N, k, _p(d2), _p(idx), _p(ws), ws_bytes, _p(visited), _p(passes), _stream()), "dicp_knn_grid_query")
        ctx.save_for_backward(x)
        ctx.grid, ctx.ws, ctx.k, ctx.shape = grid, ws, k, (N, n, cx, m, cy)
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)
        return d2, idx

    @staticmethod
    def backward(ctx, g_d2, _g_idx):
        return _backward(ctx, g_d2, 8)


def grid_knn(xb, yb, rx, grid, k, visited=None, passes=None):
    """The k nearest rows of yb (N,m,c), whose density grid is `grid`, for every row of xb (N,n,c) -> (d2, idx) (N,n,k)"""
    xkeys, xperm = grid.order(xb.detach(), rx)
    return _GridKnn.apply(xb, yb, grid, xkeys, xperm, k, visited, passes)


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


def ball_query(x, y, radius, k=16, x_rows=None, y_rows=None, return_counts=False, _visited=None):
    """The rows of y within `radius` of every row of x: the nearest k of them, and optionally how many there are, exactly.

    x, y, x_rows, y_rows: as knn_points -- one cloud each (n, c) and (m, c); a padded batch each (N, n, c) and (N, m, c) with optional
        integer row counts (N,); or two lists of N clouds.  Both in the same form, dtype (float32 or float64) and device; columns 0:3 are
        used.  CPU tensors are computed on the GPU and returned on the CPU.
    radius: one radius for the whole call, a Python float or a 0-d tensor, finite and > 0.  It is converted to the points' dtype T first,
        then r2 = radius_T * radius_T, rounded in T.  (A 0-d tensor that lives on the device is not read back, so it cannot be checked
        here: a value that is not a finite number > 0 in T gives every query count 0.)
    k: an int in [1, 32].

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
    neighbours nor counts carries any.  The forward and the x-gradient (written once per row) are bit-reproducible; the y-gradient sums
    through float atomics, as knn_points' does, and is not, from run to run.

    y is sorted into a cell grid (CellGrid: the cell edge is the search half-width, a little above the radius, enlarged per cloud on the
    device where extent / radius would not fit a 64-bit key), the queries are processed in the order of its cells, and every query scans
    only the cells its ball can touch.  Nothing is read back from the device: with device tensors and device (or no) row counts a call
    is kernels only.
    """
    _clouds._check_k(k, "ball_query", K_MIN, K_MAX)
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
    d2, idx, counts = _BallQuery.apply(xb, yb, grid, xkeys, xperm, k, _visited)
    return _clouds.restore(form, on_cpu, n, lens, [(ROW, d2), (ROW, idx)] + ([(ROW, counts)] if return_counts else []))
