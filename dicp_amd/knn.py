"""Differentiable k nearest neighbours between two clouds, and the Chamfer distance built from them.

Exact results on the GPU (libdicp_hip.so: dicp_knn_points / dicp_knn_points_backward), without the (n, m) distance matrix:

    from dicp_amd.knn import knn_points, chamfer_distance
    d2, idx = knn_points(x, y, k=8)               # squared distances and row indices of y, (..., n, k)
    loss = chamfer_distance(out["pc"], target[..., :3])
"""

import torch

from . import _clouds, _lib
from ._clouds import ROW, K_MIN, K_MAX, METHODS, _check_deterministic, _check_method      # noqa: F401  (METHODS: part of this module's interface)
from ._grid import CellGrid, grad_y_det, grid_knn
from ._ops import _DT, _p

REDUCTIONS = ("mean", "sum", "none")
DET_HUB = 4             # KNN_DET_HUB (csrc/dicp_knn_det.h): with deterministic=True a list of more than DET_HUB chunks of 64 entries is summed by a whole wave


class _Prepared:
    """One cloud sorted by raw x (dicp_sweep_sort + dicp_sweep_build, frame = NULL): keys (N,m_pad), perm (N,m_pad) int32, tgs4 (N,m_pad,4)."""

    def __init__(self, pts, rows):
        N, m, c = pts.shape
        self.pts, self.rows, self.shape = pts, rows, (N, m, c)
        dt = _DT[pts.dtype]
        lib = _lib.load()
        m_pad = lib.dicp_padded_targets(m)
        dev = pts.device
        self.keys = torch.empty((N, m_pad), dtype=pts.dtype, device=dev)
        self.perm = torch.empty((N, m_pad), dtype=torch.int32, device=dev)
        self.tgs4 = torch.empty((N, m_pad, 4), dtype=pts.dtype, device=dev)
        sb = lib.dicp_sweep_sort_scratch_bytes(dt, N, m_pad)
        scratch = torch.empty(sb, dtype=torch.uint8, device=dev) if sb else None
        _lib.call("dicp_sweep_sort", dev, dt, _p(pts), c, None, _p(rows), N, m, m_pad, _p(self.keys), _p(self.perm), 0, None, None, _p(scratch), sb)
        _lib.call("dicp_sweep_build", dev, dt, _p(pts), c, None, _p(rows), _p(self.perm), N, m, m_pad, _p(self.tgs4), None, 0)


class _KnnPoints(torch.autograd.Function):
    """(x (N,n,c), y (N,m,c)) -> (d2 (N,n,k), idx (N,n,k) int64) on prepared clouds: one library call per direction on the current stream."""

    @staticmethod
    def forward(ctx, x, y, px, py, k, det=False):
        N, n, cx = px.shape
        m, cy = py.shape[1], py.shape[2]
        dt = _DT[x.dtype]
        lib = _lib.load()
        ws_bytes = lib.dicp_knn_points_workspace_bytes(dt, N, n, m, k, 0)
        d2 = torch.empty((N, n, k), dtype=x.dtype, device=x.device)
        idx = torch.empty((N, n, k), dtype=torch.int64, device=x.device)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        _lib.call("dicp_knn_points", x.device, dt, _p(px.tgs4), _p(px.perm), _p(px.rows), n, _p(py.keys), _p(py.tgs4), _p(py.perm), _p(py.rows), m,
                  N, k, _p(d2), _p(idx), _p(ws), ws_bytes, None)
        ctx.px, ctx.py, ctx.ws, ctx.k, ctx.det = px, py, ws, k, det
        if det:                                             # the y-gradient walks the inverted index of idx over the caller's x and y
            ctx.save_for_backward(x, y, idx)
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)
        return d2, idx

    @staticmethod
    def backward(ctx, g_d2, _g_idx):
        if g_d2 is None:
            return (None,) * 6
        px, py, k = ctx.px, ctx.py, ctx.k
        N, n, cx = px.shape
        m, cy = py.shape[1], py.shape[2]
        want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_x or want_y):
            return (None,) * 6
        dtype = g_d2.dtype
        dt = _DT[dtype]
        lib = _lib.load()
        dev = g_d2.device
        gx = torch.empty((N, n, cx), dtype=dtype, device=dev) if want_x else None
        if ctx.det:                                         # the x-gradient from the same kernel (grad_y = NULL), the y-gradient stored once
            g_d2 = g_d2.contiguous()
            if want_x:
                _lib.call("dicp_knn_points_backward", dev, dt, _p(g_d2), _p(px.tgs4), _p(px.perm), _p(px.rows), n, cx, _p(py.tgs4), _p(py.perm), m, cy,
                          N, k, _p(ctx.ws), _p(gx), None, None, 0)
            x, y, idx = ctx.saved_tensors
            gy = grad_y_det(g_d2, idx, py.rows, x, y) if want_y else None
            return gx, gy, None, None, None, None
        gy = torch.empty((N, m, cy), dtype=dtype, device=dev) if want_y else None
        g_bytes = lib.dicp_knn_points_workspace_bytes(dt, N, n, m, k, 1) if want_y else 0
        gws = torch.empty(g_bytes, dtype=torch.uint8, device=dev) if want_y else None
        g_d2 = g_d2.contiguous()
        _lib.call("dicp_knn_points_backward", dev, dt, _p(g_d2), _p(px.tgs4), _p(px.perm), _p(px.rows), n, cx, _p(py.tgs4), _p(py.perm), m, cy,
                  N, k, _p(ctx.ws), _p(gx), _p(gy), _p(gws), g_bytes)
        return gx, gy, None, None, None, None


def _search(xb, yb, px, py, k, n, det=False):
    d2, idx = _KnnPoints.apply(xb, yb, px, py, k, det)
    return d2[:, :n], idx[:, :n]


def knn_points(x, y, k=8, x_rows=None, y_rows=None, method="walk", _visited=None, _passes=None, deterministic=False):
    """The k nearest rows of y for every row of x, exactly, with gradients of the squared distances.

    x, y: one cloud each (n, c) and (m, c); a padded batch each (N, n, c) and (N, m, c) with optional integer row counts x_rows / y_rows (N,);
        or two lists of N clouds.  Both in the same form, dtype (float32 or float64) and device; columns 0:3 are used (pt2pl rows with normals
        can be passed as they are).  CPU tensors are computed on the GPU and returned on the CPU.  Row counts are checked on the host only
        when they are CPU tensors.
    k: an int in [1, 32].
    method: "walk" (the default) searches along the x-sorted cloud; "grid" sorts y into a cell grid whose cell edge is chosen on the device
        from y's own density (CellGrid.by_density, about two rows per cell) and lets every query grow a box of cells until its k-th
        distance is proved final (dicp_knn_grid_build / dicp_knn_grid_query; the proof is csrc/dicp_gridknn.h).  Both are exact and return
        the same bits; they differ in speed only (README, "Nearest neighbours and Chamfer distance").
    deterministic: a bool (anything else is a ValueError before any device work); see "Gradients".

    Definition: d2(i, j) = (xx + yy) + zz with dx = y_j.x - x_i.x, xx = dx * dx (and so on), in the inputs' dtype, as separate roundings.  The
    candidates of query i of cloud b are the rows j < y_rows[b] whose d2 is finite; the result is the first k_eff = min(k, #candidates) of
    them in (d2, index) order.  Slots beyond k_eff, and query rows at or past x_rows[b], hold d2 = +inf and idx = -1.

    Returns (d2, idx): (n, k) for single clouds, (N, n, k) for a batch, lists of (n_b, k) for lists; d2 in x's dtype, idx int64.

    Gradients flow from d2 to x[..., :3] (sum_j 2 g_ij (x_i - y_idx)) and y[..., :3] (-sum 2 g_ij (x_i - y_l) over the entries with idx = l);
    other columns, pad rows and idx = -1 entries get zero, and the choice of neighbours gets none.  The forward and the x-gradient are
    bit-reproducible.  The y-gradient is by default added with float atomics: the order, and so the last bits, can differ from run to
    run.  With method="grid" the backward is ball_query's (dicp_ball_query_backward), with the same properties.

    With deterministic=True the forward and the x-gradient are the default call's, bit for bit, and the y-gradient is summed per row l
    of y over the row's list in the inverted index of the returned idx (group.invert_neighbors, built once inside the backward and only
    when y needs a gradient: the entries with idx = l in ascending i k + s), in chunks of 64 list positions -- each chunk from +0 by
    plain additions, the chunks' partials added in order to a total that starts at +0, a single chunk as it is.  A term is
    -(2 g_is)(x_i - y_l) per coordinate, formed in float64 and rounded once to the inputs' dtype (the value the atomics add); an entry
    whose cotangent is 0 has no term.  Every element is stored once -- no zero fill, no atomics: bit-reproducible, and the same bytes
    under "walk" and "grid" (dicp_knn_backward_y_det).
    """
    _clouds._check_k(k, "knn_points", K_MIN, K_MAX)
    _check_method(method, "knn_points")
    _check_deterministic(deterministic, "knn_points")
    form, on_cpu, lens, n, _, xb, yb, rx, ry = _clouds.pair(x, y, x_rows, y_rows, "knn_points")
    if method == "grid":
        d2, idx = grid_knn(xb, yb, rx, CellGrid.by_density(yb.detach(), ry), k, _visited, _passes, deterministic)
    else:
        px, py = _Prepared(xb.detach(), rx), _Prepared(yb.detach(), ry)
        d2, idx = _KnnPoints.apply(xb, yb, px, py, k, deterministic)
    return _clouds.restore(form, on_cpu, n, lens, [(ROW, d2), (ROW, idx)])


def _direction(d2, rows, n):
    """(N,n,1) nearest squared distances -> (N,) their mean over each cloud's first rows[b] queries; 0 for an empty query side"""
    N = d2.shape[0]
    dev = d2.device
    cnt = rows.to(torch.int64) if rows is not None else torch.full((N,), n, dtype=torch.int64, device=dev)
    live = torch.arange(n, device=dev)[None, :] < cnt[:, None]
    s = torch.where(live, d2[..., 0], torch.zeros((), dtype=d2.dtype, device=dev)).sum(1)
    return s / cnt.clamp(min=1).to(d2.dtype)


def chamfer_distance(x, y, x_rows=None, y_rows=None, reduction="mean", method="walk", deterministic=False):
    """Chamfer distance between two clouds: for cloud b, mean_{i < n_b} d2(x_i, NN_y(x_i)) + mean_{j < m_b} d2(y_j, NN_x(y_j)).

    x, y and the row counts: as knn_points.  d2 as knn_points defines it (squared, in the inputs' dtype).  A direction whose query side is
    empty contributes 0; a non-empty query side facing an empty cloud gives +inf (the minimum over an empty set).
    reduction: "mean" or "sum" over the batch (a scalar), or "none" ((N,), one value per cloud; (1,) for single clouds).

    Each cloud is sorted once and searched in both directions (two k = 1 searches of knn_points); gradients flow to x[..., :3] and y[..., :3]
    as knn_points describes: by default through the same float atomics.
    method: as knn_points.  "grid" builds the cell grid of each cloud once and searches each direction on the other cloud's grid.
    deterministic: a bool, as knn_points.  True makes both searches deterministic: each cloud's gradient is then the sum of two tensors
        that were each written once (its x-gradient as the query side of one search, its y-gradient in the order of summation knn_points
        describes as the target side of the other), and a two-term float add is commutative: the gradients are bit-reproducible
        whatever order autograd adds them in.
    """
    if not isinstance(reduction, str) or reduction not in REDUCTIONS:
        raise ValueError("chamfer_distance: reduction must be one of %s, got %r" % (", ".join(REDUCTIONS), reduction))
    _check_method(method, "chamfer_distance")
    _check_deterministic(deterministic, "chamfer_distance")
    form, on_cpu, _, n, m, xb, yb, rx, ry = _clouds.pair(x, y, x_rows, y_rows, "chamfer_distance")
    if method == "grid":
        gx, gy = CellGrid.by_density(xb.detach(), rx), CellGrid.by_density(yb.detach(), ry)
        d_xy, d_yx = grid_knn(xb, yb, rx, gy, 1, det=deterministic)[0][:, :n], grid_knn(yb, xb, ry, gx, 1, det=deterministic)[0][:, :m]
    else:
        px, py = _Prepared(xb.detach(), rx), _Prepared(yb.detach(), ry)
        d_xy, _ = _search(xb, yb, px, py, 1, n, deterministic)
        d_yx, _ = _search(yb, xb, py, px, 1, m, deterministic)
    per = _direction(d_xy, rx, n) + _direction(d_yx, ry, m)
    out = per if reduction == "none" else (per.mean() if reduction == "mean" else per.sum())
    return out.cpu() if on_cpu else out
