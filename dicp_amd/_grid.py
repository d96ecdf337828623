"""The cell grid of a batch of clouds and the exact k-nearest-neighbour search on it: what ball.py (fixed-radius neighbours) and knn.py
(knn_points / chamfer_distance with method="grid") share.  libdicp_hip.so: dicp_ball_grid_build / dicp_knn_grid_build / dicp_knn_grid_query /
dicp_ball_query_backward -- and the deterministic y-gradient of all three searches, dicp_knn_backward_y_det."""
import torch

from . import _lib
from ._ops import _DT, _p
from .group import _invert


def grad_y_det(g_d2, idx, y_rows, x, y):
    """The y-gradient of a search with deterministic=True -> (N,m,cy): the inverted index of the search's own idx output (N,n,k) int64,
    built here -- once, and only because y needs a gradient -- then dicp_knn_backward_y_det, which stores every element once.  g_d2
    (N,n,k), x (N,n,cx), y (N,m,cy) contiguous: the caller's arrays, the same for the walk, the grid and ball_query."""
    N, n, k = idx.shape
    m, cy = y.shape[1], y.shape[2]
    off, slots = _invert(idx, y_rows, m)
    gy = torch.empty((N, m, cy), dtype=g_d2.dtype, device=g_d2.device)
    _lib.call("dicp_knn_backward_y_det", g_d2.device, _DT[g_d2.dtype], _p(g_d2), _p(idx), _p(y_rows), _p(x), x.shape[2], n, _p(y), cy, m, N, k,
              _p(off), _p(slots), _p(gy))
    return gy


class CellGrid:
    """The cell grid of every cloud of a batch (dicp_ball_grid_build): the rows sorted by a 64-bit cell key.

    pts (N,m,c) on the device, rows (N,) int32 or None, radius a (1,) device tensor of pts' dtype.  keys (N,P) int64 holding the unsigned
    keys, perm (N,P) int32, rows4 (N,P,4) the live rows packed in sorted order, plans the per-cloud origin / cell edges / key widths /
    live-row count, all chosen on the device.  P = dicp_ball_grid_slots(m); memory is O(m) per cloud whatever extent / radius is.
    """

    def __init__(self, pts, rows, radius):
        self._build("dicp_ball_grid_build", pts, rows, _p(radius), None)

    @classmethod
    def by_density(cls, pts, rows):
        """The grid without a radius (dicp_knn_grid_build), for the k-NN search: the cell edge is chosen per cloud on the device from the
        number and the bounds of its live rows, about two rows per cell of the bounding box (csrc/dicp_gridknn.h)."""
        self = cls.__new__(cls)
        self._build("dicp_knn_grid_build", pts, rows)
        return self

    def _build(self, name, pts, rows, *edge_from):
        """edge_from: what the entry point takes between m and plans (dicp_ball_grid_build: the radius, and no order_by)"""
        N, m, c = pts.shape
        lib = _lib.load()
        dev = pts.device
        self.shape, self.rows = (N, m, c), rows
        self.slots = P = lib.dicp_ball_grid_slots(m)
        self.plans = torch.empty((N, lib.dicp_ball_plan_bytes()), dtype=torch.uint8, device=dev)
        self.keys = torch.empty((N, P), dtype=torch.int64, device=dev)
        self.perm = torch.empty((N, P), dtype=torch.int32, device=dev)
        self.rows4 = torch.empty((N, P, 4), dtype=pts.dtype, device=dev)
        _lib.call(name, dev, _DT[pts.dtype], _p(pts), c, _p(rows), N, m, *edge_from, _p(self.plans), _p(self.keys), _p(self.perm), _p(self.rows4))

    def order(self, x, x_rows):
        """-> (keys (N,Pn) int64, perm (N,Pn) int32): the rows of x (N,n,c) in the order of this grid's cells"""
        N, n, c = x.shape
        Pn = _lib.load().dicp_ball_grid_slots(n)
        keys = torch.empty((N, Pn), dtype=torch.int64, device=x.device)
        perm = torch.empty((N, Pn), dtype=torch.int32, device=x.device)
        _lib.call("dicp_ball_grid_build", x.device, _DT[x.dtype], _p(x), c, _p(x_rows), N, n, None, _p(self.plans), None, _p(keys), _p(perm), None)
        return keys, perm


def _forward(ctx, name, x, y, grid, xkeys, xperm, k, counts, diagnostics, det=False):
    """The forward of a search on y's CellGrid, dicp_ball_query or dicp_knn_grid_query: -> (d2 (N,n,k), idx (N,n,k) int64) and, where the
    entry point takes them (counts: dicp_ball_query), counts (N,n) int32, with what _backward needs saved in ctx.  diagnostics: the
    optional counters the entry point takes after the workspace.  det: the backward sums the y-gradient through the inverted index of idx (it
    needs y and idx as well)."""
    N, n, cx = x.shape
    m, cy = y.shape[1], y.shape[2]
    dt = _DT[x.dtype]
    dev = x.device
    ws_bytes = _lib.load().dicp_ball_query_workspace_bytes(dt, N, n, k)
    outs = (torch.empty((N, n, k), dtype=x.dtype, device=dev), torch.empty((N, n, k), dtype=torch.int64, device=dev))
    if counts:
        outs += (torch.empty((N, n), dtype=torch.int32, device=dev),)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.call(name, dev, dt, _p(x), cx, n, _p(xkeys), _p(xperm), _p(grid.plans), _p(grid.keys), _p(grid.perm), _p(grid.rows4), m, N, k,
              *[_p(t) for t in outs], _p(ws), ws_bytes, *[_p(t) for t in diagnostics])
    if det:
        ctx.save_for_backward(x, y, outs[1])
    else:
        ctx.save_for_backward(x)
    ctx.grid, ctx.ws, ctx.k, ctx.shape, ctx.det = grid, ws, k, (N, n, cx, m, cy), det
    ctx.mark_non_differentiable(*outs[1:])
    ctx.set_materialize_grads(False)
    return outs


def _backward(ctx, g_d2, n_inputs):
    """dicp_ball_query_backward from what a forward on a CellGrid saved: the gradients of x and y, None for the other inputs.  With
    ctx.det it gives the x-gradient only (grad_y = NULL: the same kernel, the same bits) and grad_y_det the y-gradient."""
    nothing = (None,) * n_inputs
    want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if g_d2 is None or not (want_x or want_y):
        return nothing
    x = ctx.saved_tensors[0]
    N, n, cx, m, cy = ctx.shape
    grid = ctx.grid
    dtype, dev = g_d2.dtype, g_d2.device
    gx = torch.empty((N, n, cx), dtype=dtype, device=dev) if want_x else None
    g_d2 = g_d2.contiguous()
    if ctx.det:
        if want_x:
            _lib.call("dicp_ball_query_backward", dev, _DT[dtype], _p(g_d2), _p(x), cx, n, _p(grid.rows4), _p(grid.perm), m, cy, N, ctx.k,
                      _p(ctx.ws), _p(gx), None)
        gy = grad_y_det(g_d2, ctx.saved_tensors[2], grid.rows, x, ctx.saved_tensors[1]) if want_y else None
        return (gx, gy) + nothing[2:]
    gy = torch.empty((N, m, cy), dtype=dtype, device=dev) if want_y else None
    _lib.call("dicp_ball_query_backward", dev, _DT[dtype], _p(g_d2), _p(x), cx, n, _p(grid.rows4), _p(grid.perm), m, cy, N, ctx.k,
              _p(ctx.ws), _p(gx), _p(gy))
    return (gx, gy) + nothing[2:]


class _GridKnn(torch.autograd.Function):
    """(x (N,n,c), y (N,m,c)) -> (d2 (N,n,k), idx (N,n,k) int64): the k nearest rows on y's density grid (dicp_knn_grid_query); the
    backward is ball_query's."""

    @staticmethod
    def forward(ctx, x, y, grid, xkeys, xperm, k, visited, passes, det=False):
        return _forward(ctx, "dicp_knn_grid_query", x, y, grid, xkeys, xperm, k, False, (visited, passes), det)

    @staticmethod
    def backward(ctx, g_d2, _g_idx):
        return _backward(ctx, g_d2, 9)


def grid_knn(xb, yb, rx, grid, k, visited=None, passes=None, det=False):
    """The k nearest rows of yb (N,m,c), whose density grid is `grid`, for every row of xb (N,n,c) -> (d2, idx) (N,n,k).  det: the
    y-gradient is summed through the inverted index of idx (knn_points' deterministic=True)"""
    xkeys, xperm = grid.order(xb.detach(), rx)
    return _GridKnn.apply(xb, yb, grid, xkeys, xperm, k, visited, passes, det)
