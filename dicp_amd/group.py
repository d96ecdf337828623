"""Differentiable neighbourhood features: gather, pool and interpolate a feature table through the index tensors of the neighbour operators.

The feature half of the point-cloud front end, on the GPU (libdicp_hip.so: dicp_group_* / dicp_pool_* / dicp_interpolate_*; the per-slot
rules: csrc/dicp_group.h).  ball_query and knn_points return (..., n, k) indices whose empty slots hold -1; these functions read them as they
are -- no clamp, no expanded index, no mask, no read-back:

    from dicp_amd.group import group_points, pool_neighbors, interpolate_features
    d2, idx = ball_query(centres, cloud, 0.5, k=16, x_rows=crows, y_rows=rows)
    grouped = group_points(table, idx, rows=rows, centers=centres)        # (N, n, 16, C): table[idx] with columns 0:3 relative to the centre
    pooled = pool_neighbors(per_point, idx, "max", rows=rows)             # (N, n, C): the maximum over each neighbourhood, nothing grouped
    d2, idx3 = knn_points(points, centres, k=3, y_rows=crows)
    w = interpolate_features(w_centres, idx3, d2, rows=crows)              # (N, n_points, 1): PointNet++'s feature propagation

A slot (b, i, s) is LIVE when 0 <= idx[b, i, s] < rows[b] (< m without rows, < m_b for lists): decided by one unsigned compare in the
kernel, so nothing is read out of range whatever idx holds and nothing is checked on the host.  Every other slot is empty: -1, any other
negative value, anything at or past the row count.  Query rows past their cloud's count need no argument: the neighbour operators give
them -1 in every slot.

Nothing is read back from the device and every launch is on the current stream, the zero fill of a gradient table included (a kernel,
not a memset node).  With device tensors and device rows (or none) a call, forward and backward, can be captured in a graph
(torch.cuda.graph) and replayed on new data in the same buffers: tests/test_gpu_group_graph.py does so for the three operators.
"""
import math

import torch
from torch.autograd.function import once_differentiable

from . import _clouds, _lib
from ._clouds import ROW, K_MIN, K_MAX
from ._ops import _DT, _p, _stream, _on


def _dims(f, idx):
    return f.shape[0], idx.shape[1], f.shape[1], idx.shape[2], f.shape[2]            # N, n, m, k, C


# (the forwards call the library directly: of their 30 us, _lib.call's lookup by name and extra frame are 0.5, profiles/r18_dispatch_host_time.txt)
def _i64(idx):
    return 1 if idx.dtype == torch.int64 else 0


class _Group(torch.autograd.Function):
    """(features (N,m,C), idx (N,n,k), rows, centers (N,n,Cc) or None) -> (N,n,k,C): one library call per direction."""

    @staticmethod
    def forward(ctx, f, idx, rows, cen):
        N, n, m, k, C = _dims(f, idx)
        Cc = cen.shape[2] if cen is not None else 0
        out = torch.empty((N, n, k, C), dtype=f.dtype, device=f.device)
        with _on(f.device):
            _lib.check(_lib.load().dicp_group_forward(_DT[f.dtype], _p(f), _p(idx), _i64(idx), _p(rows), _p(cen), Cc, N, n, m, k, C, _p(out), _stream()),
                       "dicp_group_forward")
        ctx.save_for_backward(idx, rows)
        ctx.dims, ctx.Cc = (N, n, m, k, C), Cc
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        want_f, want_c = ctx.needs_input_grad[0], ctx.needs_input_grad[3] and ctx.Cc > 0
        if g is None or not (want_f or want_c):
            return None, None, None, None
        idx, rows = ctx.saved_tensors
        N, n, m, k, C = ctx.dims
        g = g.contiguous()
        gf = torch.empty((N, m, C), dtype=g.dtype, device=g.device) if want_f else None
        gc = torch.empty((N, n, ctx.Cc), dtype=g.dtype, device=g.device) if want_c else None
        _lib.call("dicp_group_backward", g.device, _DT[g.dtype], _p(g), _p(idx), _i64(idx), _p(rows), ctx.Cc, N, n, m, k, C, _p(gf), _p(gc))
        return gf, None, None, gc


class _Interpolate(torch.autograd.Function):
    """(features (N,m,C), idx (N,n,k), d2 (N,n,k), rows) -> (N,n,C); the backward recomputes the weights from d2 and the saved output."""

    @staticmethod
    def forward(ctx, f, idx, d2, rows, eps):
        N, n, m, k, C = _dims(f, idx)
        out = torch.empty((N, n, C), dtype=f.dtype, device=f.device)
        with _on(f.device):
            _lib.check(_lib.load().dicp_interpolate_forward(_DT[f.dtype], _p(f), _p(idx), _i64(idx), _p(rows), _p(d2), eps, N, n, m, k, C, _p(out), _stream()),
                       "dicp_interpolate_forward")
        ctx.save_for_backward(f, idx, d2, rows, out)
        ctx.dims, ctx.eps = (N, n, m, k, C), eps
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        want_f, want_d = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        if g is None or not (want_f or want_d):
            return None, None, None, None, None
        f, idx, d2, rows, out = ctx.saved_tensors
        N, n, m, k, C = ctx.dims
        g = g.contiguous()
        gf = torch.empty((N, m, C), dtype=g.dtype, device=g.device) if want_f else None
        gd = torch.empty((N, n, k), dtype=g.dtype, device=g.device) if want_d else None
        _lib.call("dicp_interpolate_backward", g.device, _DT[g.dtype], _p(g), _p(f), _p(out), _p(idx), _i64(idx), _p(rows), _p(d2), ctx.eps, N, n, m, k, C,
                  _p(gf), _p(gd))
        return gf, None, gd, None, None


class _Pool(torch.autograd.Function):
    """(features (N,m,C), idx (N,n,k), rows, reduce) -> out (N,n,C), argmax (N,n,C) int32 (max; otherwise an empty tensor), counts (N,n) int32:
    one library call per direction."""

    @staticmethod
    def forward(ctx, f, idx, rows, reduce):
        N, n, m, k, C = _dims(f, idx)
        out = torch.empty((N, n, C), dtype=f.dtype, device=f.device)
        amax = torch.empty((N, n, C) if reduce == _lib.POOL_MAX else (0,), dtype=torch.int32, device=f.device)
        counts = torch.empty((N, n), dtype=torch.int32, device=f.device)
        with _on(f.device):
            _lib.check(_lib.load().dicp_pool_forward(_DT[f.dtype], _p(f), _p(idx), _i64(idx), _p(rows), reduce, N, n, m, k, C, _p(out),
                                                     _p(amax) if reduce == _lib.POOL_MAX else None, _p(counts), _stream()), "dicp_pool_forward")
        ctx.save_for_backward(idx, rows, amax, counts)
        ctx.dims, ctx.reduce = (N, n, m, k, C), reduce
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(amax, counts)
        return out, amax, counts

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _ga, _gc):
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        idx, rows, amax, counts = ctx.saved_tensors
        N, n, m, k, C = ctx.dims
        g = g.contiguous()
        gf = torch.empty((N, m, C), dtype=g.dtype, device=g.device)
        _lib.call("dicp_pool_backward", g.device, _DT[g.dtype], _p(g), _p(idx), _i64(idx), _p(rows), ctx.reduce,
                  _p(amax) if ctx.reduce == _lib.POOL_MAX else None, _p(counts), N, n, m, k, C, _p(gf))
        return gf, None, None, None


def _front(features, idx, rows, what):
    """The checks the two functions share (no device is touched) -> (form, features batch, rows, idx batch, lengths of idx's list)"""
    form, fb, rows, _ = _clouds.check(features, rows, what, "features", "rows", min_cols=1)
    ib, lens = _clouds.check_slots(idx, what, "idx", (form, fb), True, K_MIN, K_MAX)
    return form, fb, rows, ib, lens


def _rows_like(t, what, name, form, ib, lens, cols_max=None):
    """A (..., n, c) argument that goes with idx row by row (centers) -> its batch (N,n,c)"""
    cform, cb, _, clens = _clouds.check(t, None, what, name, min_cols=1)
    if cform != form:
        raise ValueError("%s: %s must have the form of the features (single clouds, padded batches or lists), got %s and %s" % (what, name, cform, form))
    if cb.shape[0] != ib.shape[0]:
        raise ValueError("%s: %s and idx must hold the same number of clouds, got %d and %d" % (what, name, cb.shape[0], ib.shape[0]))
    if cb.shape[1] != ib.shape[1] or clens != lens:
        raise ValueError("%s: %s needs one row per row of idx, got shapes %s and %s" % (what, name, tuple(cb.shape), tuple(ib.shape)))
    if cols_max is not None and cb.shape[2] > cols_max:
        raise ValueError("%s: %s has %d columns, the features only %d" % (what, name, cb.shape[2], cols_max))
    return cb


def _same(what, name, t, fb):
    if t.dtype != fb.dtype:
        raise ValueError("%s: %s and the features must have one dtype, got %s and %s" % (what, name, t.dtype, fb.dtype))
    if t.device != fb.device:
        raise ValueError("%s: %s and the features must be on one device, got %s and %s" % (what, name, t.device, fb.device))


def group_points(features, idx, rows=None, centers=None):
    """The feature rows that idx names, one block of k rows per query: out[..., i, s, :] = features[..., idx[..., i, s], :].

    features: one table (m, C), a padded batch (N, m, C) with optional integer counts rows (N,) of live rows, or a list of (m_b, C) tables;
        float32 or float64, C >= 1.  CPU tensors are computed on the GPU and returned on the CPU.
    idx: (n, k), (N, n, k) or a list of (n_b, k), the same form as features; int64 (what ball_query / knn_points return) or int32, read by
        the kernels as it is; 1 <= k <= 32.  A slot is live when 0 <= idx < rows[b] (m, m_b): see the module's docstring.
    centers: optional (n, Cc), (N, n, Cc) or a list of (n_b, Cc) with 1 <= Cc <= C, features' form, dtype and device.  On live slots
        columns 0:Cc have centers[..., i, :] subtracted (one rounding), the other columns pass through: PointNet++'s grouped_xyz - new_xyz
        on an (xyz | features) table in one call.

    Returns (n, k, C), (N, n, k, C) or a list of (n_b, k, C): the gathered rows on live slots, 0 on empty ones -- exact.

    Gradients: features[..., j, :] receives the sum of the cotangent rows of the live slots with idx = j, added with float atomics (the
    order, and so the last bits, can differ from run to run); rows nobody points at get exactly 0.  centers[..., i, c] receives
    -(the sum over the live slots of query i, in slot order), written once: bit-reproducible.  Empty slots contribute nothing whatever
    cotangent arrives there, NaN and inf included.

    Nothing is read back and every launch is on the current stream: a call on device tensors (device or no rows) is kernels only; a list
    or CPU rows add a host-to-device copy.  Capture in a graph: see the module's docstring.
    """
    what = "group_points"
    form, fb, rows, ib, lens = _front(features, idx, rows, what)
    cb = None
    if centers is not None:
        cb = _rows_like(centers, what, "centers", form, ib, lens, cols_max=fb.shape[2])
        _same(what, "centers", cb, fb)
    on_cpu, f_d, rows_d = _clouds.place(fb, rows)
    out = _Group.apply(f_d, ib.to(f_d.device).contiguous(), rows_d, cb.to(f_d.device).contiguous() if cb is not None else None)
    return _clouds.restore(form, on_cpu, ib.shape[1], lens, [(ROW, out)])[0]


_REDUCE = {"sum": _lib.POOL_SUM, "mean": _lib.POOL_MEAN, "max": _lib.POOL_MAX}


def pool_neighbors(features, idx, reduce="max", rows=None, return_argmax=False, return_counts=False):
    """The maximum, mean or sum of the feature rows that idx names, per query and channel, over the k slots: group_points followed by a
    reduction over the slots, without the (N, n, k, C) tensor in between (nor its n k C gradient atomics: n C for the maximum).

    features, idx, rows: as group_points -- one table (m, C) with idx (n, k), a padded batch with rows, or lists; float32 or float64;
        int64 or int32 indices read as they are, 1 <= k <= 32; C >= 1.  A slot is live when 0 <= idx < rows[b] (m, m_b).
    reduce: "max", "mean" or "sum".
    return_argmax: also return argmax (..., n, C) int32 (only with "max").  return_counts: also return counts (..., n) int32, the number
        of live slots of each query.

    Definition, per query i and channel c, every operation in the features' dtype T, over the live slots in slot order:
      "sum":  acc = 0, then acc = acc + features[idx_s, c] for each live slot: plain additions, bit-reproducible.
      "mean": that sum, then one division by T(count); within (k + 2) u sum_s |features[idx_s, c]| / count of the exact mean, u the unit
              roundoff of T.
      "max":  best starts at the first live slot's value; a later value v replaces it when v > best -- on ties the lowest slot wins, and
              +0 and -0 tie -- or when v is NaN and best is not: a NaN propagates as in torch.max, and the first NaN's slot is the
              argmax.  argmax[i, c] is the TABLE ROW idx[i, s] of the winning slot, not s.  +-inf are ordinary values.  Exact.
      A query without a live slot gives out = 0, argmax = -1, counts = 0; so do the rows of a list's or a padded batch's queries past
      their cloud's count (the neighbour operators give them -1 in every slot).

    There is no centers argument: rounding to nearest is monotone, so max_s(f_s - centre) = max_s(f_s) - centre exactly -- subtract the
    centre's row from the pooled result.  (For the mean and the sum the two orders differ by roundings; group_points(centers=) is there.)

    Returns out (n, C), (N, n, C) or a list of (n_b, C); with return_argmax and / or return_counts a tuple (out, argmax, counts) of the
    ones asked for, in this order.

    Gradients: "max": features[argmax[i, c], c] receives g[i, c]; "sum": every live slot's row receives g[i, :]; "mean": every live
    slot's row receives g[i, c] / T(count), one rounding.  All three add with float atomics, as group_points (the last bits can differ
    from run to run); rows nobody points at get exactly 0.  A query without a live slot contributes nothing whatever cotangent arrives
    there, NaN and inf included.  argmax and counts carry no gradient.

    Nothing is read back, every launch is on the current stream, and nothing is checked on the host beyond shapes; capture in a graph:
    see the module's docstring.
    """
    what = "pool_neighbors"
    if not isinstance(reduce, str) or reduce not in _REDUCE:
        raise ValueError("%s: reduce must be 'max', 'mean' or 'sum', got %r" % (what, reduce))
    if return_argmax and reduce != "max":
        raise ValueError("%s: return_argmax needs reduce='max', got %r" % (what, reduce))
    form, fb, rows, ib, lens = _front(features, idx, rows, what)
    on_cpu, f_d, rows_d = _clouds.place(fb, rows)
    out, amax, counts = _Pool.apply(f_d, ib.to(f_d.device).contiguous(), rows_d, _REDUCE[reduce])
    outs = [(ROW, out)] + ([(ROW, amax)] if return_argmax else []) + ([(ROW, counts)] if return_counts else [])
    res = _clouds.restore(form, on_cpu, ib.shape[1], lens, outs)
    return res if len(res) > 1 else res[0]


def interpolate_features(features, idx, d2, eps=1e-8, rows=None):
    """Inverse-distance interpolation of feature rows (PointNet++'s feature propagation): out[i] = sum_s w_s features[idx[i, s]].

    features, idx, rows: as group_points -- the table of the m centres and, per query, the k centres to interpolate between.
    d2: (..., n, k) squared distances in the features' dtype, the d2 of knn_points(x, centres, k=3) or of ball_query; it carries gradients.
        A slot is live when its index is live AND its d2 is finite (the neighbour operators pad with +inf).
    eps: a Python float, finite and > 0 after rounding to the features' dtype T.

    Definition, every operation in T and in slot order over the live slots: r_s = 1 / (d2_s + eps), R = sum_s r_s, w_s = r_s / R,
    out[i, :] = sum_s w_s features[idx_s, :]; 0 without a live slot.  Several exact zeros of d2 share the weight equally.  d2 >= 0 is
    expected: what d2 + eps <= 0 gives is unspecified (and so is a d2 so large that 1 / d2 underflows to 0).  Each output is within
    (2k + 8) u sum_s w_s |features[idx_s, c]| of the exact value of this expression on the same inputs, u the unit roundoff of T.

    Returns (n, C), (N, n, C) or a list of (n_b, C).

    Gradients: features[idx_s, :] receives w_s times the cotangent row (float atomics, as group_points'); d2 receives
    -(r_s^2 / R) sum_c g[i, c] (features[idx_s, c] - out[i, c]) on live slots and 0 elsewhere, written once per slot: bit-reproducible.
    Through d2 the gradient reaches both clouds by knn_points' / ball_query's own backward.  The backward recomputes r and R from d2 and
    keeps the forward's output; no per-slot weight is stored.
    """
    what = "interpolate_features"
    if isinstance(eps, bool) or not isinstance(eps, (int, float)):
        raise ValueError("%s: eps must be a float, finite and > 0, got %r" % (what, eps))
    if isinstance(eps, int) and abs(eps) > 2 ** 1023:
        raise ValueError("%s: eps must be finite and > 0, got %r" % (what, eps))
    eps = float(eps)
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError("%s: eps must be finite and > 0, got %r" % (what, eps))
    form, fb, rows, ib, lens = _front(features, idx, rows, what)
    eps_t = float(torch.tensor(eps, dtype=fb.dtype))
    if not (math.isfinite(eps_t) and eps_t > 0.0):
        raise ValueError("%s: eps must be finite and > 0 in %s, got %r" % (what, fb.dtype, eps))
    db, dlens = _clouds.check_slots(d2, what, "d2", (form, fb), False, K_MIN, K_MAX)
    if db.shape != ib.shape or dlens != lens:
        raise ValueError("%s: d2 and idx must have one shape, got %s and %s" % (what, tuple(db.shape), tuple(ib.shape)))
    on_cpu, f_d, rows_d = _clouds.place(fb, rows)
    out = _Interpolate.apply(f_d, ib.to(f_d.device).contiguous(), db.to(f_d.device).contiguous(), rows_d, eps_t)
    return _clouds.restore(form, on_cpu, ib.shape[1], lens, [(ROW, out)])[0]
