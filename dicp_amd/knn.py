"""Differentiable k nearest neighbours between two clouds, and the Chamfer distance built from them.

Exact results on the GPU (libdicp_hip.so: dicp_knn_points / dicp_knn_points_backward), without the (n, m) distance matrix:

    from dicp_amd.knn import knn_points, chamfer_distance
    d2, idx = knn_points(x, y, k=8)               # squared distances and row indices of y, (..., n, k)
    loss = chamfer_distance(out["pc"], target[..., :3])
"""

import torch

from . import _lib
from ._ops import _DT, _p, _stream, _on, compute_device

K_MIN, K_MAX = 1, 32
REDUCTIONS = ("mean", "sum", "none")


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
        with _on(dev):
            st = _stream()
            _lib.check(lib.dicp_sweep_sort(dt, _p(pts), c, None, _p(rows), N, m, m_pad, _p(self.keys), _p(self.perm), 0, None, None,
                                           _p(scratch), sb, st), "dicp_sweep_sort")
            _lib.check(lib.dicp_sweep_build(dt, _p(pts), c, None, _p(rows), _p(self.perm), N, m, m_pad, _p(self.tgs4), None, 0, st),
                       "dicp_sweep_build")


class _KnnPoints(torch.autograd.Function):
    """(x (N,n,c), y (N,m,c)) -> (d2 (N,n,k), idx (N,n,k) int64) on prepared clouds: one library call per direction on the current stream."""

    @staticmethod
    def forward(ctx, x, y, px, py, k):
        N, n, cx = px.shape
        m, cy = py.shape[1], py.shape[2]
        dt = _DT[x.dtype]
        lib = _lib.load()
        ws_bytes = lib.dicp_knn_points_workspace_bytes(dt, N, n, m, k, 0)
        d2 = torch.empty((N, n, k), dtype=x.dtype, device=x.device)
        idx = torch.empty((N, n, k), dtype=torch.int64, device=x.device)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        with _on(x.device):
            _lib.check(lib.dicp_knn_points(dt, _p(px.tgs4), _p(px.perm), _p(px.rows), n, _p(py.keys), _p(py.tgs4), _p(py.perm), _p(py.rows), m,
                                           N, k, _p(d2), _p(idx), _p(ws), ws_bytes, None, _stream()), "dicp_knn_points")
        ctx.px, ctx.py, ctx.ws, ctx.k = px, py, ws, k
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)
        return d2, idx

    @staticmethod
    def backward(ctx, g_d2, _g_idx):
        if g_d2 is None:
            return None, None, None, None, None
        px, py, k = ctx.px, ctx.py, ctx.k
        N, n, cx = px.shape
        m, cy = py.shape[1], py.shape[2]
        want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_x or want_y):
            return None, None, None, None, None
        dtype = g_d2.dtype
        dt = _DT[dtype]
        lib = _lib.load()
        dev = g_d2.device
        gx = torch.empty((N, n, cx), dtype=dtype, device=dev) if want_x else None
        gy = torch.empty((N, m, cy), dtype=dtype, device=dev) if want_y else None
        g_bytes = lib.dicp_knn_points_workspace_bytes(dt, N, n, m, k, 1) if want_y else 0
        gws = torch.empty(g_bytes, dtype=torch.uint8, device=dev) if want_y else None
        g_d2 = g_d2.contiguous()
        with _on(dev):
            _lib.check(lib.dicp_knn_points_backward(dt, _p(g_d2), _p(px.tgs4), _p(px.perm), _p(px.rows), n, cx, _p(py.tgs4), _p(py.perm), m, cy,
                                                    N, k, _p(ctx.ws), _p(gx), _p(gy), _p(gws), g_bytes, _stream()), "dicp_knn_points_backward")
        return gx, gy, None, None, None


def _err(msg):
    raise ValueError(msg)


def _check_k(k, what):
    if isinstance(k, bool) or not isinstance(k, int) or not (K_MIN <= k <= K_MAX):
        _err("%s: k must be an int in [%d, %d], got %r" % (what, K_MIN, K_MAX, k))


def _check_points(t, name, what):
    if not isinstance(t, torch.Tensor):
        _err("%s: %s must be a tensor, got %s" % (what, name, type(t).__name__))
    if t.dtype not in _DT:
        _err("%s: %s must be float32 or float64, got %s" % (what, name, t.dtype))
    if t.dim() < 1 or t.shape[-1] < 3:
        _err("%s: %s needs at least 3 columns (x, y, z), got shape %s" % (what, name, tuple(t.shape)))


def _batch(t, rows, name, what):
    """-> (form, (N,m,c) batch, rows or None, lengths of a list or None); ValueError for anything invalid"""
    if isinstance(t, (list, tuple)):
        if not t:
            _err("%s: %s is an empty list" % (what, name))
        for i, c in enumerate(t):
            _check_points(c, "%s[%d]" % (name, i), what)
            if c.dim() != 2:
                _err("%s: %s[%d] must be (m_b, c), got shape %s" % (what, name, i, tuple(c.shape)))
        if len({c.shape[1] for c in t}) != 1 or len({c.dtype for c in t}) != 1 or len({c.device for c in t}) != 1:
            _err("%s: the clouds of %s need one column count, dtype and device" % (what, name))
        if rows is not None:
            _err("%s: %s is a list: its row counts come from the list itself" % (what, name))
        lens = [c.shape[0] for c in t]
        batch = torch.nn.utils.rnn.pad_sequence(list(t), batch_first=True)
        return "list", batch, torch.tensor(lens, dtype=torch.int32), lens
    _check_points(t, name, what)
    if t.dim() == 2:
        if rows is not None:
            _err("%s: %s_rows needs a padded batch (N, m, c)" % (what, name))
        return "single", t.unsqueeze(0), None, None
    if t.dim() != 3:
        _err("%s: %s must be (m, c), (N, m, c) or a list of (m_b, c), got shape %s" % (what, name, tuple(t.shape)))
    if rows is not None:
        r = torch.as_tensor(rows)
        if r.dtype.is_floating_point or r.dtype.is_complex or r.dtype == torch.bool or r.dim() != 1 or r.numel() != t.shape[0]:
            _err("%s: %s_rows must be %d integer counts" % (what, name, t.shape[0]))
        if not r.is_cuda and r.numel() and (int(r.min()) < 0 or int(r.max()) > t.shape[1]):
            _err("%s: %s_rows must lie in [0, %d]" % (what, name, t.shape[1]))
        rows = r
    return "batch", t, rows, None


def _inputs(x, y, x_rows, y_rows, what):
    """Validates both arguments (before any device work) and moves them to the device: -> (form, on_cpu, lens_x, n, m, x (N,n',c), y (N,m',c),
    x_rows, y_rows) with n', m' >= 1 (an empty side is padded to one row with a row count of 0) and c in {3, 6}."""
    fx, bx, rx, lx = _batch(x, x_rows, "x", what)
    fy, by, ry, ly = _batch(y, y_rows, "y", what)
    if fx != fy:
        _err("%s: x and y must have the same form (single clouds, padded batches or lists), got %s and %s" % (what, fx, fy))
    if bx.dtype != by.dtype:
        _err("%s: x and y must have one dtype, got %s and %s" % (what, bx.dtype, by.dtype))
    if bx.device != by.device:
        _err("%s: x and y must be on one device, got %s and %s" % (what, bx.device, by.device))
    if bx.shape[0] != by.shape[0]:
        _err("%s: x and y must hold the same number of clouds, got %d and %d" % (what, bx.shape[0], by.shape[0]))
    if bx.shape[0] < 1:
        _err("%s: empty batch" % what)
    on_cpu = not bx.is_cuda
    dev = compute_device() if on_cpu else bx.device

    def put(b, r):
        b = b.to(dev)
        if b.shape[-1] not in (3, 6):
            b = b[..., :3]
        N, m = b.shape[0], b.shape[1]
        if m == 0:                                      # the library needs a row: one pad row, no row taking part
            b = torch.zeros((N, 1, b.shape[2]), dtype=b.dtype, device=dev) + b.sum() * 0
            r = torch.zeros(N, dtype=torch.int32)
        r = torch.as_tensor(r).to(device=dev, dtype=torch.int32).contiguous() if r is not None else None
        return b.contiguous(), r
    bx_d, rx_d = put(bx, rx)
    by_d, ry_d = put(by, ry)
    return fx, on_cpu, lx, bx.shape[1], by.shape[1], bx_d, by_d, rx_d, ry_d


def _search(xb, yb, px, py, k, n):
    d2, idx = _KnnPoints.apply(xb, yb, px, py, k)
    return d2[:, :n], idx[:, :n]


def knn_points(x, y, k=8, x_rows=None, y_rows=None):
    """The k nearest rows of y for every row of x, exactly, with gradients of the squared distances.

    x, y: one cloud each (n, c) and (m, c); a padded batch each (N, n, c) and (N, m, c) with optional integer row counts x_rows / y_rows (N,);
        or two lists of N clouds.  Both in the same form, dtype (float32 or float64) and device; columns 0:3 are used (pt2pl rows with normals
        can be passed as they are).  CPU tensors are computed on the GPU and returned on the CPU.  Row counts are checked on the host only
        when they are CPU tensors.
    k: an int in [1, 32].

    Definition: d2(i, j) = (xx + yy) + zz with dx = y_j.x - x_i.x, xx = dx * dx (and so on), in the inputs' dtype, as separate roundings.  The
    candidates of query i of cloud b are the rows j < y_rows[b] whose d2 is finite; the result is the first k_eff = min(k, #candidates) of
    them in (d2, index) order.  Slots beyond k_eff, and query rows at or past x_rows[b], hold d2 = +inf and idx = -1.

    Returns (d2, idx): (n, k) for single clouds, (N, n, k) for a batch, lists of (n_b, k) for lists; d2 in x's dtype, idx int64.

    Gradients flow from d2 to x[..., :3] (sum_j 2 g_ij (x_i - y_idx)) and y[..., :3] (-sum 2 g_ij (x_i - y_l) over the entries with idx = l);
    other columns, pad rows and idx = -1 entries get zero, and the choice of neighbours gets none.  The forward and the x-gradient are
    bit-reproducible; the y-gradient sums through float atomics and is not, from run to run.
    """
    _check_k(k, "knn_points")
    form, on_cpu, lens, n, _, xb, yb, rx, ry = _inputs(x, y, x_rows, y_rows, "knn_points")
    px, py = _Prepared(xb.detach(), rx), _Prepared(yb.detach(), ry)
    d2, idx = _search(xb, yb, px, py, k, n)
    if on_cpu:
        d2, idx = d2.cpu(), idx.cpu()
    if form == "list":
        return [d2[b, :lens[b]] for b in range(len(lens))], [idx[b, :lens[b]] for b in range(len(lens))]
    if form == "single":
        return d2[0], idx[0]
    return d2, idx


def _direction(d2, rows, n):
    """(N,n,1) nearest squared distances -> (N,) their mean over each cloud's first rows[b] queries; 0 for an empty query side"""
    N = d2.shape[0]
    dev = d2.device
    cnt = rows.to(torch.int64) if rows is not None else torch.full((N,), n, dtype=torch.int64, device=dev)
    live = torch.arange(n, device=dev)[None, :] < cnt[:, None]
    s = torch.where(live, d2[..., 0], torch.zeros((), dtype=d2.dtype, device=dev)).sum(1)
    return s / cnt.clamp(min=1).to(d2.dtype)


def chamfer_distance(x, y, x_rows=None, y_rows=None, reduction="mean"):
    """Chamfer distance between two clouds: for cloud b, mean_{i < n_b} d2(x_i, NN_y(x_i)) + mean_{j < m_b} d2(y_j, NN_x(y_j)).

    x, y and the row counts: as knn_points.  d2 as knn_points defines it (squared, in the inputs' dtype).  A direction whose query side is
    empty contributes 0; a non-empty query side facing an empty cloud gives +inf (the minimum over an empty set).
    reduction: "mean" or "sum" over the batch (a scalar), or "none" ((N,), one value per cloud; (1,) for single clouds).

    Each cloud is sorted once and searched in both directions (two k = 1 searches of knn_points); gradients flow to x[..., :3] and y[..., :3]
    as knn_points describes, and through the same float atomics.
    """
    if not isinstance(reduction, str) or reduction not in REDUCTIONS:
        _err("chamfer_distance: reduction must be one of %s, got %r" % (", ".join(REDUCTIONS), reduction))
    form, on_cpu, _, n, m, xb, yb, rx, ry = _inputs(x, y, x_rows, y_rows, "chamfer_distance")
    px, py = _Prepared(xb.detach(), rx), _Prepared(yb.detach(), ry)
    d_xy, _ = _search(xb, yb, px, py, 1, n)
    d_yx, _ = _search(yb, xb, py, px, 1, m)
    per = _direction(d_xy, rx, n) + _direction(d_yx, ry, m)
    out = per if reduction == "none" else (per.mean() if reduction == "mean" else per.sum())
    return out.cpu() if on_cpu else out
