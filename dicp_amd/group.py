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
not a memset node).

The gradient into a feature table is a scatter: by default it is added with float atomics, whose order -- and so the last bits -- can
differ from run to run.  deterministic=True (or inverse=) on the three operators sums it through an inverted index instead, per
destination row in a fixed order, so that every gradient of this module is bit-reproducible; invert_neighbors builds that index, which
is also the reverse neighbour list of an index tensor in its own right:

    inv = invert_neighbors(idx, m, rows=rows)                             # offsets (N, m + 1), slots (N, n k): who names row j
    pooled = pool_neighbors(per_point, idx, "max", rows=rows, inverse=inv)
    grouped = group_points(table, idx, rows=rows, inverse=inv)            # layers that share one idx pay for the build once

With device tensors and device rows (or none) a call, forward and backward, can be captured in a graph
(torch.cuda.graph) and replayed on new data in the same buffers: tests/test_gpu_group_graph.py does so for the three operators.
"""
import math

import torch
from torch.autograd.function import once_differentiable

from . import _clouds, _lib
from ._clouds import ROW, K_MIN, K_MAX
from ._ops import _DT, _p, _stream, _on, compute_device

DET_CHUNK = 64          # GROUP_DET_CHUNK (csrc/dicp_inverse.h): the list positions summed from +0 before their partial joins the total


def _dims(f, idx):
    return f.shape[0], idx.shape[1], f.shape[1], idx.shape[2], f.shape[2]            # N, n, m, k, C


# (the forwards call the library directly: of their 30 us, _lib.call's lookup by name and extra frame are 0.5, profiles/r18_dispatch_host_time.txt)
def _i64(idx):
    return 1 if idx.dtype == torch.int64 else 0


def _invert(idx, rows, m):
    """idx (N,n,k) contiguous on the GPU, rows (N,) int32 there or None -> offsets (N,m+1), slots (N,n*k) int32: kernels on the current stream"""
    N, n, k = idx.shape
    lib = _lib.load()
    need = lib.dicp_invert_neighbors_workspace_bytes(N, n, m, k)
    if need == 0:
        raise ValueError("invert_neighbors: n * k must stay below 2^31 per cloud, got n = %d, k = %d (N = %d, m = %d)" % (n, k, N, m))
    offsets = torch.empty((N, m + 1), dtype=torch.int32, device=idx.device)
    slots = torch.empty((N, n * k), dtype=torch.int32, device=idx.device)
    ws = torch.empty(need, dtype=torch.uint8, device=idx.device)
    _lib.call("dicp_invert_neighbors", idx.device, _p(idx), _i64(idx), _p(rows), N, n, m, k, _p(offsets), _p(slots), _p(ws), need)
    return offsets, slots


def _index_of(ctx, idx, rows, off, slots):
    """the inverted index of a deterministic backward: the caller's, or built now -- once, and only because the features need a gradient"""
    if off is not None:
        return off, slots
    return _invert(idx, rows, ctx.dims[2])


class _Group(torch.autograd.Function):
    """(features (N,m,C), idx (N,n,k), rows, centers (N,n,Cc) or None) -> (N,n,k,C): one library call per direction."""

    @staticmethod
    def forward(ctx, f, idx, rows, cen, det=False, off=None, slots=None):
        N, n, m, k, C = _dims(f, idx)
        Cc = cen.shape[2] if cen is not None else 0
        out = torch.empty((N, n, k, C), dtype=f.dtype, device=f.device)
        with _on(f.device):
            _lib.check(_lib.load().dicp_group_forward(_DT[f.dtype], _p(f), _p(idx), _i64(idx), _p(rows), _p(cen), Cc, N, n, m, k, C, _p(out), _stream()),
                       "dicp_group_forward")
        ctx.save_for_backward(idx, rows, off, slots)
        ctx.dims, ctx.Cc, ctx.det = (N, n, m, k, C), Cc, det
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        want_f, want_c = ctx.needs_input_grad[0], ctx.needs_input_grad[3] and ctx.Cc > 0
        if g is None or not (want_f or want_c):
            return (None,) * 7
        idx, rows, off, slots = ctx.saved_tensors
        N, n, m, k, C = ctx.dims
        g = g.contiguous()
        gf = torch.empty((N, m, C), dtype=g.dtype, device=g.device) if want_f else None
        gc = torch.empty((N, n, ctx.Cc), dtype=g.dtype, device=g.device) if want_c else None
        if not ctx.det:
            _lib.call("dicp_group_backward", g.device, _DT[g.dtype], _p(g), _p(idx), _i64(idx), _p(rows), ctx.Cc, N, n, m, k, C, _p(gf), _p(gc))
            return gf, None, None, gc, None, None, None
        if want_c:
            _lib.call("dicp_group_backward", g.device, _DT[g.dtype], _p(g), _p(idx), _i64(idx), _p(rows), ctx.Cc, N, n, m, k, C, None, _p(gc))
        if want_f:
            off, slots = _index_of(ctx, idx, rows, off, slots)
            _lib.call("dicp_group_backward_det", g.device, _DT[g.dtype], _p(g), _p(idx), _i64(idx), _p(rows), N, n, m, k, C, _p(off), _p(slots), _p(gf))
        return gf, None, None, gc, None, None, None


class _Interpolate(torch.autograd.Function):
    """(features (N,m,C), idx (N,n,k), d2 (N,n,k), rows) -> (N,n,C); the backward recomputes the weights from d2 and the saved output."""

    @staticmethod
    def forward(ctx, f, idx, d2, rows, eps, det=False, off=None, slots=None):
        N, n, m, k, C = _dims(f, idx)
        out = torch.empty((N, n, C), dtype=f.dtype, device=f.device)
        with _on(f.device):
            _lib.check(_lib.load().dicp_interpolate_forward(_DT[f.dtype], _p(f), _p(idx), _i64(idx), _p(rows), _p(d2), eps, N, n, m, k, C, _p(out), _stream()),
                       "dicp_interpolate_forward")
        ctx.save_for_backward(f, idx, d2, rows, out, off, slots)
        ctx.dims, ctx.eps, ctx.det = (N, n, m, k, C), eps, det
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        want_f, want_d = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        if g is None or not (want_f or want_d):
            return (None,) * 8
        f, idx, d2, rows, out, off, slots = ctx.saved_tensors
        N, n, m, k, C = ctx.dims
        g = g.contiguous()
        gf = torch.empty((N, m, C), dtype=g.dtype, device=g.device) if want_f else None
        gd = torch.empty((N, n, k), dtype=g.dtype, device=g.device) if want_d else None
        if not ctx.det:
            _lib.call("dicp_interpolate_backward", g.device, _DT[g.dtype], _p(g), _p(f), _p(out), _p(idx), _i64(idx), _p(rows), _p(d2), ctx.eps, N, n, m, k, C,
                      _p(gf), _p(gd))
            return gf, None, gd, None, None, None, None, None
        if want_d:
            _lib.call("dicp_interpolate_backward", g.device, _DT[g.dtype], _p(g), _p(f), _p(out), _p(idx), _i64(idx), _p(rows), _p(d2), ctx.eps, N, n, m, k, C,
                      None, _p(gd))
        if want_f:
            off, slots = _index_of(ctx, idx, rows, off, slots)
            _lib.call("dicp_interpolate_backward_det", g.device, _DT[g.dtype], _p(g), _p(idx), _i64(idx), _p(rows), _p(d2), ctx.eps, N, n, m, k, C,
                      _p(off), _p(slots), _p(gf))
        return gf, None, gd, None, None, None, None, None


class _Pool(torch.autograd.Function):
    """(features (N,m,C), idx (N,n,k), rows, reduce) -> out (N,n,C), argmax (N,n,C) int32 (max; otherwise an empty tensor), counts (N,n) int32:
    one library call per direction."""

    @staticmethod
    def forward(ctx, f, idx, rows, reduce, det=False, off=None, slots=None):
        N, n, m, k, C = _dims(f, idx)
        out = torch.empty((N, n, C), dtype=f.dtype, device=f.device)
        amax = torch.empty((N, n, C) if reduce == _lib.POOL_MAX else (0,), dtype=torch.int32, device=f.device)
        counts = torch.empty((N, n), dtype=torch.int32, device=f.device)
        with _on(f.device):
            _lib.check(_lib.load().dicp_pool_forward(_DT[f.dtype], _p(f), _p(idx), _i64(idx), _p(rows), reduce, N, n, m, k, C, _p(out),
                                                     _p(amax) if reduce == _lib.POOL_MAX else None, _p(counts), _stream()), "dicp_pool_forward")
        ctx.save_for_backward(idx, rows, amax, counts, off, slots)
        ctx.dims, ctx.reduce, ctx.det = (N, n, m, k, C), reduce, det
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(amax, counts)
        return out, amax, counts

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _ga, _gc):
        if g is None or not ctx.needs_input_grad[0]:
            return (None,) * 7
        idx, rows, amax, counts, off, slots = ctx.saved_tensors
        N, n, m, k, C = ctx.dims
        g = g.contiguous()
        gf = torch.empty((N, m, C), dtype=g.dtype, device=g.device)
        if not ctx.det:
            _lib.call("dicp_pool_backward", g.device, _DT[g.dtype], _p(g), _p(idx), _i64(idx), _p(rows), ctx.reduce,
                      _p(amax) if ctx.reduce == _lib.POOL_MAX else None, _p(counts), N, n, m, k, C, _p(gf))
            return gf, None, None, None, None, None, None
        off, slots = _index_of(ctx, idx, rows, off, slots)
        _lib.call("dicp_pool_backward_det", g.device, _DT[g.dtype], _p(g), _p(idx), _i64(idx), _p(rows), ctx.reduce,
                  _p(amax) if ctx.reduce == _lib.POOL_MAX else None, _p(counts), N, n, m, k, C, _p(off), _p(slots), _p(gf))
        return gf, None, None, None, None, None, None


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


def _inverse_arg(what, deterministic, inverse, form, fb, rows, ib, lens):
    """deterministic= / inverse= of the three operators, checked before any device work -> (det, offsets (N,m+1), slots (N,n*k)) with the
    pair as a batch on idx's device, or (det, None, None).  inverse: what invert_neighbors returned for the same idx and rows, in the
    same form; it implies det.  A list's pairs are padded as its clouds are: offsets continued with the cloud's live count, slots with -1."""
    if not isinstance(deterministic, bool):
        raise ValueError("%s: deterministic must be True or False, got %r" % (what, deterministic))
    if inverse is None:
        return deterministic, None, None
    N, m, n, k = fb.shape[0], fb.shape[1], ib.shape[1], ib.shape[2]
    if n * k >= 2 ** 31:
        raise ValueError("%s: n * k must stay below 2^31 per cloud, got n = %d, k = %d" % (what, n, k))
    if form == "list":
        if not isinstance(inverse, (list, tuple)) or len(inverse) != N or not all(isinstance(p, (list, tuple)) and len(p) == 2 for p in inverse):
            raise ValueError("%s: inverse must be the list of %d (offsets, slots) pairs that invert_neighbors returns for lists" % (what, N))
        pairs = [tuple(p) for p in inverse]
        shapes = [((int(rows[b]) + 1,), (lens[b] * k,)) for b in range(N)]
    else:
        if not isinstance(inverse, (list, tuple)) or len(inverse) != 2:
            raise ValueError("%s: inverse must be the (offsets, slots) pair that invert_neighbors returns" % what)
        pairs = [tuple(inverse)]
        shapes = [((m + 1,), (n * k,)) if form == "single" else ((N, m + 1), (N, n * k))]
    for (o, sl), (so, ss) in zip(pairs, shapes):
        for name, t in (("offsets", o), ("slots", sl)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
                raise ValueError("%s: inverse's %s must be an int32 tensor, got %s" % (what, name, t.dtype if isinstance(t, torch.Tensor) else type(t).__name__))
            if t.device != ib.device:
                raise ValueError("%s: inverse and idx must be on one device, got %s and %s" % (what, t.device, ib.device))
        if tuple(o.shape) != so or tuple(sl.shape) != ss:
            raise ValueError("%s: inverse must have shapes %s and %s for these features and idx, got %s and %s" % (what, so, ss, tuple(o.shape), tuple(sl.shape)))
    if form == "list":
        off = torch.stack([torch.cat([o, o[-1:].expand(m + 1 - o.shape[0])]) for o, _ in pairs])
        slots = torch.stack([torch.nn.functional.pad(sl, (0, n * k - sl.shape[0]), value=-1) for _, sl in pairs])
        return True, off, slots
    return True, pairs[0][0].reshape(N, m + 1), pairs[0][1].reshape(N, n * k)


def _to(t, dev):
    return t.to(dev).contiguous() if t is not None else None


def _same(what, name, t, fb):
    if t.dtype != fb.dtype:
        raise ValueError("%s: %s and the features must have one dtype, got %s and %s" % (what, name, t.dtype, fb.dtype))
    if t.device != fb.device:
        raise ValueError("%s: %s and the features must be on one device, got %s and %s" % (what, name, t.device, fb.device))


def group_points(features, idx, rows=None, centers=None, deterministic=False, inverse=None):
    """The feature rows that idx names, one block of k rows per query: out[..., i, s, :] = features[..., idx[..., i, s], :].

    features: one table (m, C), a padded batch (N, m, C) with optional integer counts rows (N,) of live rows, or a list of (m_b, C) tables;
        float32 or float64, C >= 1.  CPU tensors are computed on the GPU and returned on the CPU.
    idx: (n, k), (N, n, k) or a list of (n_b, k), the same form as features; int64 (what ball_query / knn_points return) or int32, read by
        the kernels as it is; 1 <= k <= 32.  A slot is live when 0 <= idx < rows[b] (m, m_b): see the module's docstring.
    centers: optional (n, Cc), (N, n, Cc) or a list of (n_b, Cc) with 1 <= Cc <= C, features' form, dtype and device.  On live slots
        columns 0:Cc have centers[..., i, :] subtracted (one rounding), the other columns pass through: PointNet++'s grouped_xyz - new_xyz
        on an (xyz | features) table in one call.

    Returns (n, k, C), (N, n, k, C) or a list of (n_b, k, C): the gathered rows on live slots, 0 on empty ones -- exact.

    deterministic, inverse: see "Gradients".  deterministic must be a bool; inverse the pair (a list's pairs) invert_neighbors returned for
        the same idx and rows, in the same form and on idx's device -- anything else is a ValueError before any device work.

    Gradients: features[..., j, :] receives the sum of the cotangent rows of the live slots with idx = j.  By default it is added with
    float atomics (the order, and so the last bits, can differ from run to run).  With deterministic=True it is summed per row j over the
    row's list in the inverted index (invert_neighbors: the live slots naming j in ascending i k + s), in chunks of DET_CHUNK = 64 list
    positions -- each chunk from +0 by plain additions, the chunks' partials added in order to a total that starts at +0, a single chunk
    as it is -- and stored once: bit-reproducible, no zero fill, no atomics.  The backward builds the index once, lazily, and only when
    the features need a gradient; inverse= passes a prebuilt one (and implies deterministic), so that layers sharing one idx pay for the
    build once.  Either way rows nobody points at get exactly 0.  centers[..., i, c] receives
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
    det, off, slots = _inverse_arg(what, deterministic, inverse, form, fb, rows, ib, lens)
    on_cpu, f_d, rows_d = _clouds.place(fb, rows)
    if not det:
        out = _Group.apply(f_d, ib.to(f_d.device).contiguous(), rows_d, cb.to(f_d.device).contiguous() if cb is not None else None)
    else:
        out = _Group.apply(f_d, ib.to(f_d.device).contiguous(), rows_d, cb.to(f_d.device).contiguous() if cb is not None else None,
                           True, _to(off, f_d.device), _to(slots, f_d.device))
    return _clouds.restore(form, on_cpu, ib.shape[1], lens, [(ROW, out)])[0]


_REDUCE = {"sum": _lib.POOL_SUM, "mean": _lib.POOL_MEAN, "max": _lib.POOL_MAX}


def pool_neighbors(features, idx, reduce="max", rows=None, return_argmax=False, return_counts=False, deterministic=False, inverse=None):
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
    from run to run), or, with deterministic=True / inverse= (as group_points: same arguments, same order of summation), sum the same
    terms per row over its list in the inverted index and store once: bit-reproducible.  Under "max" a query whose slots name one row
    several times still sends g[i, c] once.  Rows nobody points at get exactly 0.  A query without a live slot contributes nothing
    whatever cotangent arrives there, NaN and inf included.  argmax and counts carry no gradient.

    Nothing is read back, every launch is on the current stream, and nothing is checked on the host beyond shapes; capture in a graph:
    see the module's docstring.
    """
    what = "pool_neighbors"
    if not isinstance(reduce, str) or reduce not in _REDUCE:
        raise ValueError("%s: reduce must be 'max', 'mean' or 'sum', got %r" % (what, reduce))
    if return_argmax and reduce != "max":
        raise ValueError("%s: return_argmax needs reduce='max', got %r" % (what, reduce))
    form, fb, rows, ib, lens = _front(features, idx, rows, what)
    det, off, slots = _inverse_arg(what, deterministic, inverse, form, fb, rows, ib, lens)
    on_cpu, f_d, rows_d = _clouds.place(fb, rows)
    if not det:
        out, amax, counts = _Pool.apply(f_d, ib.to(f_d.device).contiguous(), rows_d, _REDUCE[reduce])
    else:
        out, amax, counts = _Pool.apply(f_d, ib.to(f_d.device).contiguous(), rows_d, _REDUCE[reduce], True, _to(off, f_d.device), _to(slots, f_d.device))
    outs = [(ROW, out)] + ([(ROW, amax)] if return_argmax else []) + ([(ROW, counts)] if return_counts else [])
    res = _clouds.restore(form, on_cpu, ib.shape[1], lens, outs)
    return res if len(res) > 1 else res[0]


def interpolate_features(features, idx, d2, eps=1e-8, rows=None, deterministic=False, inverse=None):
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

    Gradients: features[idx_s, :] receives w_s times the cotangent row (w_s g[i, c] rounded once): float atomics by default; with
    deterministic=True / inverse= (as group_points: same arguments, same order of summation) summed per row over its list in the inverted
    index and stored once, bit-reproducible -- a slot with a non-finite d2 is in the list (the index is built from idx alone) and has no
    term.  d2 receives
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
    det, off, slots = _inverse_arg(what, deterministic, inverse, form, fb, rows, ib, lens)
    on_cpu, f_d, rows_d = _clouds.place(fb, rows)
    if not det:
        out = _Interpolate.apply(f_d, ib.to(f_d.device).contiguous(), db.to(f_d.device).contiguous(), rows_d, eps_t)
    else:
        out = _Interpolate.apply(f_d, ib.to(f_d.device).contiguous(), db.to(f_d.device).contiguous(), rows_d, eps_t, True, _to(off, f_d.device), _to(slots, f_d.device))
    return _clouds.restore(form, on_cpu, ib.shape[1], lens, [(ROW, out)])[0]


def invert_neighbors(idx, m, rows=None):
    """The inverted index of an index tensor: for every row j of the table that idx points into, the slots that name it.

    idx: (n, k), (N, n, k) or a list of (n_b, k), int64 or int32, 1 <= k <= 32 -- what ball_query / knn_points return.  CPU tensors are
        computed on the GPU and returned on the CPU.
    m: the rows of the table: an int >= 1 for (n, k) and (N, n, k); for a list, a list of ints m_b >= 0, one per cloud.
    rows: optional integer counts (N,) of live table rows, only with a padded batch (N, n, k); 0 <= rows[b] <= m.

    Definition, per cloud b with nb = rows[b] (m without rows, m_b for a list).  Slot (i, s) has the flat number q = i k + s and is LIVE
    when 0 <= idx[b, i, s] < nb -- the one unsigned compare on the index's full width that the feature operators make, so an int64 value
    such as 2^40 + 3 is empty, not row 3.  With L_b the number of live slots:
      offsets (m + 1,) int32: offsets[j] = the number of live slots naming a row < j.  offsets[0] = 0, and offsets[j] = L_b for every
          j >= nb: rows past the count have empty lists.
      slots (n k,) int32: slots[offsets[j] : offsets[j + 1]] = the q of the live slots with idx = j, in ASCENDING q; slots[L_b:] = -1.
    Row j's in-degree is offsets[j + 1] - offsets[j]; query and slot of an entry are q // k and q % k.  Both tensors are defined in full
    and exact: a stable radix sort of (row, q), the same bits on every run.  n k < 2^31 per cloud (ValueError).

    Returns (offsets (m + 1,), slots (n k,)), ((N, m + 1), (N, n k)) or a list of pairs ((m_b + 1,), (n_b k,)).  Pass the result as inverse=
    to group_points / pool_neighbors / interpolate_features called with the same idx and rows.

    Nothing is read back and every launch is on the current stream (a call on device tensors can be captured in a graph); memory is
    O(n k + m) per cloud whatever the in-degrees, all n k slots naming one row included.
    """
    what = "invert_neighbors"
    is_list = isinstance(idx, (list, tuple))
    if is_list:
        if not isinstance(m, (list, tuple)) or len(m) != len(idx) or not all(isinstance(x, int) and not isinstance(x, bool) and 0 <= x < 2 ** 31 - 1 for x in m):
            raise ValueError("%s: idx is a list: m must be a list of %d ints m_b >= 0, got %r" % (what, len(idx), m))
        if rows is not None:
            raise ValueError("%s: idx is a list: the row counts are m itself" % what)
        form, N, mm = "list", len(idx), max(max(m), 1) if m else 1
    else:
        if isinstance(m, bool) or not isinstance(m, int) or not (1 <= m < 2 ** 31 - 1):
            raise ValueError("%s: m must be an int in [1, 2^31 - 2], got %r" % (what, m))
        form = "batch" if isinstance(idx, torch.Tensor) and idx.dim() == 3 else "single"
        N, mm = (idx.shape[0] if form == "batch" else 1), m
    dev = idx[0].device if is_list and idx and isinstance(idx[0], torch.Tensor) else (idx.device if isinstance(idx, torch.Tensor) else torch.device("cpu"))
    ib, lens = _clouds.check_slots(idx, what, "idx", (form, torch.empty((max(N, 1), 0), device=dev)), True, K_MIN, K_MAX)
    n, k = ib.shape[1], ib.shape[2]
    if n * k >= 2 ** 31:
        raise ValueError("%s: n * k must stay below 2^31 per cloud, got n = %d, k = %d" % (what, n, k))
    if is_list:
        rows = torch.tensor(list(m), dtype=torch.int32)
    elif rows is not None:
        if form != "batch":
            raise ValueError("%s: rows needs a padded batch (N, n, k)" % what)
        rows = torch.as_tensor(rows)
        if rows.dtype.is_floating_point or rows.dtype.is_complex or rows.dtype == torch.bool or rows.dim() != 1 or rows.numel() != N:
            raise ValueError("%s: rows must be %d integer counts" % (what, N))
        if not rows.is_cuda and (int(rows.min()) < 0 or int(rows.max()) > m):
            raise ValueError("%s: rows must lie in [0, %d]" % (what, m))
    on_cpu = not ib.is_cuda
    cdev = compute_device() if on_cpu else ib.device
    rows_d = rows.to(device=cdev, dtype=torch.int32).reshape(-1).contiguous() if rows is not None else None
    off, slots = _invert(ib.to(cdev).contiguous(), rows_d, mm)
    if on_cpu:
        off, slots = off.cpu(), slots.cpu()
    if form == "list":
        return [(off[b, :m[b] + 1], slots[b, :lens[b] * k]) for b in range(N)]
    return (off[0], slots[0]) if form == "single" else (off, slots)
