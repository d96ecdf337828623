"""Outlier removal for batches of clouds: a differentiable mask compaction and the two standard filters on top of it.

Everything runs on the GPU (libdicp_hip.so: dicp_select_rows / dicp_select_rows_backward / dicp_outlier_stats, and the searches of
dicp_amd.ball and dicp_amd.knn).  The result is a zero-padded batch with per-cloud row counts, the form `estimate_normals(..., rows=)` and
`ICP.icp(..., source_rows=, target_rows=)` take:

    from dicp_amd.filter import select_rows, radius_outlier_removal, statistical_outlier_removal
    cent, rows = voxel_downsample(scan, 0.1)
    cent, rows = statistical_outlier_removal(cent, k=16, std_ratio=2.0, rows=rows)
    nrm = estimate_normals(cent, k=16, rows=rows)
    target = torch.cat((cent, nrm), dim=-1)       # -> ICP(icp_type='pt2pl').icp(..., target_rows=rows)
"""
import math
import numbers

import torch

from . import _clouds, _lib
from ._clouds import ROW, CLOUD, VOXEL
from ._ops import _DT, _p, _workspace
from .ball import ball_query, _check_radius
from .knn import knn_points

SELECT_TILE = 1024                  # rows per tile of the compaction kernels (csrc/dicp_filter.h)
SELECT_SCAN_THREADS = 256           # tiles per pass of the per-cloud scan
K_MIN, K_MAX = 1, 31                # the k of statistical_outlier_removal: the search runs with k + 1 slots


class _Select(torch.autograd.Function):
    """(pts (N,m,c), mask (N,m) bool, rows (N) int32 or None) -> (out (N,m,c), rows_out (N) int32, index (N,m) int64 or None): one library
    call per direction.  pos (N,m) int32, the inverse map, is written only when the points need a gradient."""

    @staticmethod
    def forward(ctx, pts, mask, rows, want_index):
        N, m, c = pts.shape
        dev = pts.device
        lib = _lib.load()
        ws_bytes = lib.dicp_select_workspace_bytes(N, m)
        ws = _workspace(ws_bytes, dev)
        out = torch.empty((N, m, c), dtype=pts.dtype, device=dev)
        rows_out = torch.empty((N,), dtype=torch.int32, device=dev)
        index = torch.empty((N, m), dtype=torch.int64, device=dev) if want_index else None
        pos = torch.empty((N, m), dtype=torch.int32, device=dev) if ctx.needs_input_grad[0] else None
        _lib.call("dicp_select_rows", dev, _DT[pts.dtype], _p(pts), c, _p(mask), _p(rows), N, m, _p(out), _p(rows_out), _p(index), _p(pos),
                  _p(ws), ws_bytes)
        ctx.save_for_backward(pos)
        ctx.shape = (N, m, c)
        ctx.mark_non_differentiable(rows_out, *([index] if want_index else []))
        ctx.set_materialize_grads(False)
        return out, rows_out, index

    @staticmethod
    def backward(ctx, g_out, _g_rows, _g_index):
        (pos,) = ctx.saved_tensors
        if g_out is None or pos is None:
            return None, None, None, None
        N, m, c = ctx.shape
        g = g_out.contiguous()
        grad = torch.empty((N, m, c), dtype=g.dtype, device=g.device)
        _lib.call("dicp_select_rows_backward", g.device, _DT[g.dtype], _p(g), _p(pos), N, m, c, _p(grad))
        return grad, None, None, None


def _compact(form, on_cpu, m, lens, x, mask, rows_d, return_index, before=(), after=()):
    """_Select on placed arguments, then the caller's form: a batch as it is (nothing is read back), a single cloud or a list cut to the
    N counts, which are read back once.  before / after: [(kind, tensor)] outputs that go before / after the index."""
    out, rows_out, index = _Select.apply(x, mask, rows_d, bool(return_index))
    outs = [(VOXEL, out), (CLOUD, rows_out)] + list(before) + ([(VOXEL, index)] if return_index else []) + list(after)
    if form == "batch":
        return tuple(t.cpu() if on_cpu else t for _, t in outs)
    return _clouds.restore(form, on_cpu, m, lens, outs, voxels=rows_out.cpu())      # the one device -> host read of the call


def select_rows(points, mask, rows=None, return_index=False):
    """The rows of every cloud that a mask keeps, in their order, as a zero-padded batch with row counts -- on the GPU, with gradients back
    to the points.

    points: (m, c), (N, m, c) or a list of (m_b, c) with c >= 1; float32 or float64.  CPU tensors are computed on the GPU and returned on
        the CPU.
    mask: torch.bool in the form of the points -- (m,), (N, m) or a list of (m_b,) -- on the same device.
    rows: optional (N,) row counts of a padded batch (rows past them are padding).
    Anything else is a ValueError before any device work.

    Definition: row r of cloud b is kept when r < rows[b] and mask[b, r].  Kept rows keep their order (the compaction is stable) and all c
    columns, bit for bit; rows_out[b] is their number; output rows at and past rows_out[b] are zero.  index[b, j] is the input row that
    output row j came from, -1 past rows_out[b].  The values are never looked at: a non-finite row that the mask keeps is kept.

    Returns (out, rows_out[, index]).  Batch input: out (N, m, c) -- the input's own width, so nothing is read back: a call on device
    tensors with device (or no) rows is kernels only and can sit in a captured region; rows_out (N,) int32; index (N, m) int64.
    Single-cloud and list input read the N counts back once, to cut the results: out (rows_out, c), rows_out a 0-d tensor, index
    (rows_out,); lists of the per-cloud ones.

    Gradient: grad_points[b, i] = grad_out[b, pos[b, i]] for a kept row and 0 for any other, pos being the inverse map the forward
    writes; every element is stored once -- no zero fill, no atomics, bit-reproducible.  The mask gets none.
    """
    form, batch, rows, lens = _clouds.check(points, rows, "select_rows", min_cols=1)
    mb = _clouds.check_mask(mask, "select_rows", "mask", (form, batch, lens))
    on_cpu, x, rows_d = _clouds.place(batch, rows)
    return _compact(form, on_cpu, batch.shape[1], lens, x, mb.to(x.device).contiguous(), rows_d, return_index)


def _check_flags(what, **flags):
    for name, v in flags.items():
        if not isinstance(v, bool):
            raise ValueError("%s: %s must be True or False, got %r" % (what, name, v))


def radius_outlier_removal(points, radius, min_neighbors, rows=None, return_mask=False, return_index=False):
    """Drop every row with fewer than min_neighbors rows of its cloud within `radius` (PCL / Open3D RadiusOutlierRemoval).

    points, rows: as select_rows, with c >= 3 (columns 0:3 are the coordinates; every column is carried along).
    radius: as ball_query takes it -- a Python float or a 0-d tensor, finite and > 0; the bound is inclusive.
    min_neighbors: an int >= 1.  A row counts itself.

    counts = ball_query(p, p, radius, k=1, x_rows=rows, y_rows=rows, return_counts=True) on the detached points; a row is kept when
    counts >= min_neighbors, and the kept rows are compacted by select_rows.  A row with a non-finite coordinate has count 0 and is
    dropped.  Returns (out, rows_out[, mask][, index]): out, rows_out and index as select_rows returns them, mask torch.bool per input
    row.  Gradients reach the kept rows through select_rows; the decision carries none.  The batch form reads nothing back.
    """
    what = "radius_outlier_removal"
    if isinstance(min_neighbors, bool) or not isinstance(min_neighbors, numbers.Integral) or min_neighbors < 1 or min_neighbors > 2 ** 31 - 1:
        raise ValueError("%s: min_neighbors must be an int >= 1, got %r" % (what, min_neighbors))
    _check_flags(what, return_mask=return_mask, return_index=return_index)
    radius = _check_radius(radius)
    form, batch, rows, lens = _clouds.check(points, rows, what)
    if isinstance(radius, float):
        r_t = float(torch.tensor(radius, dtype=batch.dtype))
        if not (math.isfinite(r_t) and r_t > 0.0):
            raise ValueError("%s: radius must be finite and > 0 in %s, got %r" % (what, batch.dtype, radius))
    on_cpu, x, rows_d = _clouds.place(batch, rows)
    xd = x.detach()
    counts = ball_query(xd, xd, radius, k=1, x_rows=rows_d, y_rows=rows_d, return_counts=True)[2]
    mask = counts >= int(min_neighbors)
    return _compact(form, on_cpu, batch.shape[1], lens, x, mask, rows_d, return_index, [(ROW, mask)] if return_mask else [])


def _outlier_stats(d2, idx, rows_d, k, std_ratio):
    """the (k + 1)-slot search of a batch against itself -> (mean_distance (N,m) float64, stats (N,3) float64, mask (N,m) bool)"""
    N, m = d2.shape[0], d2.shape[1]
    dev = d2.device
    lib = _lib.load()
    ws_bytes = lib.dicp_outlier_workspace_bytes(N, m)
    ws = _workspace(ws_bytes, dev)
    md = torch.empty((N, m), dtype=torch.float64, device=dev)
    stats = torch.empty((N, 3), dtype=torch.float64, device=dev)
    mask = torch.empty((N, m), dtype=torch.bool, device=dev)
    d2, idx = d2.contiguous(), idx.contiguous()
    _lib.call("dicp_outlier_stats", dev, _DT[d2.dtype], _p(d2), _p(idx), _p(rows_d), N, m, k, std_ratio, _p(md), _p(stats), _p(mask), _p(ws), ws_bytes)
    return md, stats, mask


def statistical_outlier_removal(points, k=16, std_ratio=2.0, rows=None, method="grid", return_mask=False, return_index=False,
                                return_mean_distance=False, return_stats=False):
    """Drop every row whose mean distance to its k nearest neighbours lies more than std_ratio standard deviations above its cloud's
    mean (PCL / Open3D StatisticalOutlierRemoval).

    points, rows: as select_rows, with c >= 3 (columns 0:3 are the coordinates; every column is carried along).
    k: an int in [1, 31].  std_ratio: a finite Python number >= 0.  method: the search, as knn_points takes it ("walk" or "grid": the same
    bits).

    Definition (what the tests pin); everything after the search is in float64:
      - (d2, idx) = knn_points(p, p, k + 1, x_rows=rows, y_rows=rows, method=method) on the detached points;
      - row i walks its k + 1 slots in order, skips the slot whose idx is i itself, and takes the first k that remain with idx >= 0,
        cnt_i of them (with exact duplicates the row itself need not be in slot 0, or in its list at all);
      - md_i = (sum of sqrt(double(d2)) over them, in slot order from +0) / cnt_i, the roots correctly rounded.  A row with cnt_i = 0 --
        a pad row, a row with a non-finite coordinate, the row of a one-row cloud -- has md_i = +inf, takes no part in the statistics and
        is dropped;
      - the statistics run over the cloud's V valid rows in row order, summed by sum64: at most 64 values are added sequentially from
        +0; a longer list is cut into consecutive chunks of 64, each summed that way, and sum64 is applied to the list of partials;
      - mean = sum64(md) / V; var = sum64(t t) / (V - 1) with t = md - mean and each product rounded on its own; std = sqrt(var), 0 when
        V < 2; thr = mean + (std_ratio std) with the product rounded first (V = 0: mean and thr are NaN);
      - row i is kept when md_i <= thr.
    Returns (out, rows_out[, mask][, index][, mean_distance][, stats]): out, rows_out and index as select_rows returns them; mask
    torch.bool and mean_distance float64 per input row; stats (N, 3) float64 = mean, std, thr ((3,) for a single cloud).  Gradients reach
    the kept rows through select_rows; the decision carries none.  No float atomics: bit-reproducible.  The batch form reads nothing back.
    """
    what = "statistical_outlier_removal"
    _clouds._check_k(k, what, K_MIN, K_MAX)
    try:
        ok = not isinstance(std_ratio, bool) and isinstance(std_ratio, numbers.Real) and math.isfinite(float(std_ratio)) and std_ratio >= 0
    except OverflowError:
        ok = False
    if not ok:
        raise ValueError("%s: std_ratio must be a finite real number >= 0, got %r" % (what, std_ratio))
    _clouds._check_method(method, what)
    _check_flags(what, return_mask=return_mask, return_index=return_index, return_mean_distance=return_mean_distance, return_stats=return_stats)
    form, batch, rows, lens = _clouds.check(points, rows, what)
    on_cpu, x, rows_d = _clouds.place(batch, rows)
    xd = x.detach()
    d2, idx = knn_points(xd, xd, k + 1, x_rows=rows_d, y_rows=rows_d, method=method)
    md, stats, mask = _outlier_stats(d2, idx, rows_d, k, float(std_ratio))
    return _compact(form, on_cpu, batch.shape[1], lens, x, mask, rows_d, return_index, [(ROW, mask)] if return_mask else [],
                    ([(ROW, md)] if return_mean_distance else []) + ([(CLOUD, stats)] if return_stats else []))
