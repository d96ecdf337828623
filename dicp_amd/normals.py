"""Differentiable surface normals for point-to-plane targets.

`ICP(icp_type='pt2pl')` takes target rows (m, 6) = xyz + unit normal.  `estimate_normals` computes those normals from the points
alone, on the GPU (libdicp_hip.so: dicp_normals_forward / dicp_normals_backward), with gradients back to the points:

    from dicp_amd.normals import estimate_normals
    nrm = estimate_normals(pts, k=16)
    target = torch.cat((pts, nrm), dim=-1)        # -> ICP(icp_type='pt2pl').icp(source, target, ...)
"""

import torch

from . import _lib
from ._ops import _DT, _p, _stream, _on, compute_device

K_MIN, K_MAX = 3, 32


class _Normals(torch.autograd.Function):
    """(N,m,c) points -> (normals (N,m,3), curvature (N,m), neighbours (N,m,k) int64 or None): one library call per direction on the current
    stream, into one allocation per direction."""

    @staticmethod
    def forward(ctx, pts, rows, vp, k, want_nbr):
        N, m, c = pts.shape
        dt = _DT[pts.dtype]
        lib = _lib.load()
        ts = pts.element_size()
        ws_bytes = lib.dicp_normals_workspace_bytes(dt, N, m, k, c, 0)
        up = lambda x: (x + 255) // 256 * 256
        o_nrm, o_curv = 0, up(N * m * 3 * ts)
        o_nbr = o_curv + up(N * m * ts)
        o_ws = o_nbr + (up(N * m * k * 8) if want_nbr else 0)
        buf = torch.empty(o_ws + ws_bytes + 256, dtype=torch.uint8, device=pts.device)
        shift = (-buf.data_ptr()) % 256                # (the caching allocator's blocks are aligned already)
        nrm = buf[shift + o_nrm: shift + o_nrm + N * m * 3 * ts].view(pts.dtype).view(N, m, 3)
        curv = buf[shift + o_curv: shift + o_curv + N * m * ts].view(pts.dtype).view(N, m)
        nbr = buf[shift + o_nbr: shift + o_nbr + N * m * k * 8].view(torch.int64).view(N, m, k) if want_nbr else None
        ws = buf[shift + o_ws:]
        with _on(pts.device):
            _lib.check(lib.dicp_normals_forward(dt, _p(pts), c, _p(rows), N, m, k, _p(vp), int(vp is not None and vp.dim() == 2),
                                                _p(nrm), _p(curv), _p(nbr), _p(ws), ws_bytes, None, _stream()), "dicp_normals_forward")
        ctx.save_for_backward(rows, vp)
        ctx.ws = ws                                     # (a view of the outputs' allocation: kept off the saved-tensor version checks)
        ctx.shape, ctx.k = (N, m, c), k
        ctx.set_materialize_grads(False)
        if nbr is not None:
            ctx.mark_non_differentiable(nbr)
        return nrm, curv, nbr

    @staticmethod
    def backward(ctx, g_nrm, g_curv, _g_nbr):
        if g_nrm is None and g_curv is None:
            return None, None, None, None, None
        rows, vp = ctx.saved_tensors
        ws = ctx.ws
        N, m, c = ctx.shape
        dtype = g_nrm.dtype if g_nrm is not None else g_curv.dtype
        dt = _DT[dtype]
        lib = _lib.load()
        ts = torch.empty((), dtype=dtype).element_size()
        g_bytes = lib.dicp_normals_workspace_bytes(dt, N, m, ctx.k, c, 1)
        n_grad = N * m * c
        buf = torch.empty(n_grad + g_bytes // ts + 128, dtype=dtype, device=ws.device)
        lead = ((-buf.data_ptr()) % 256) // ts
        grad = buf[lead: lead + n_grad].view(N, m, c)
        gws = buf[lead + (n_grad + 31) // 32 * 32:]
        g_nrm = g_nrm.contiguous() if g_nrm is not None else None
        g_curv = g_curv.contiguous() if g_curv is not None else None
        with _on(ws.device):
            _lib.check(lib.dicp_normals_backward(dt, _p(g_nrm), _p(g_curv), _p(vp), int(vp is not None and vp.dim() == 2), _p(rows), N, m, ctx.k, c,
                                                 _p(ws), _p(grad), _p(gws), gws.numel() * ts, _stream()), "dicp_normals_backward")
        return grad, None, None, None, None


def _check_k(k):
    if isinstance(k, bool) or not isinstance(k, int) or not (K_MIN <= k <= K_MAX):
        raise ValueError("estimate_normals: k must be an int in [%d, %d], got %r" % (K_MIN, K_MAX, k))


def _check_points(t, what):
    if not isinstance(t, torch.Tensor):
        raise ValueError("estimate_normals: %s must be a tensor, got %s" % (what, type(t).__name__))
    if t.dtype not in _DT:
        raise ValueError("estimate_normals: %s must be float32 or float64, got %s" % (what, t.dtype))
    if t.shape[-1] < 3:
        raise ValueError("estimate_normals: %s needs at least 3 columns (x, y, z), got shape %s" % (what, tuple(t.shape)))


def estimate_normals(points, k=16, viewpoint=None, rows=None, return_curvature=False, return_neighbors=False):
    """Unit surface normals of every point from its k nearest neighbours in its own cloud.

    points: (m, c), (N, m, c) with c >= 3 (columns 0:3 are used), or a list of (m_b, c); float32 or float64.  CPU tensors are computed on the
        GPU and returned on the CPU.
    k: 3 <= k <= 32.  rows: optional (N,) row counts of a padded batch (as ICP.icp's target_rows); rows past them are padding.
    viewpoint: None (the origin, as for a scan in its sensor frame), (3,) or (N, 3): each normal is flipped to face it.

    Definition (what the tests pin): the neighbours of point i are the k_eff = min(k, rows_b) rows of its cloud first in (d2, index) order, i itself
    among them, d2 = (dx*dx + dy*dy) + dz*dz; C = (1/k_eff) sum (q_j - mu)(q_j - mu)^T with q_j = p_j - p_i and mu = mean q; the normal is C's
    eigenvector of the smallest eigenvalue, signed so that n . (viewpoint - p_i) >= 0 (on exactly 0: its first nonzero component positive).
    k_eff < 3 and pad rows give a zero normal (pt2pl then sees no information there) and zero curvature.

    Returns normals (..., m, 3) in the points' dtype (a list for a list); with return_curvature also the surface variation
    lam0 / (lam0 + lam1 + lam2) (..., m), eigenvalues ascending, 0 for a zero trace; with return_neighbors also (..., m, k) int64 row indices,
    -1 beyond k_eff and on pad rows.

    Gradients flow to points[..., :3] (zero for the other columns); the viewpoint only picks a sign and gets none, nor do the neighbour choice
    and the sign (piecewise constant).  A point whose two smallest eigenvalues are not separated -- lam1 - lam0 <= tau (lam0 + lam1 + lam2),
    tau = 1e-6 for float32 and 1e-12 for float64 -- contributes a zero gradient instead of inf or NaN: its normal is not a function of the
    points there.  The backward sums through float atomics, so its result is not bit-reproducible from run to run.
    """
    _check_k(k)
    is_list = isinstance(points, (list, tuple))
    if is_list:
        if not points:
            raise ValueError("estimate_normals: empty list")
        for i, t in enumerate(points):
            _check_points(t, "points[%d]" % i)
            if t.dim() != 2:
                raise ValueError("estimate_normals: points[%d] must be (m_b, c), got shape %s" % (i, tuple(t.shape)))
        if len({t.shape[1] for t in points}) != 1 or len({t.dtype for t in points}) != 1 or len({t.device for t in points}) != 1:
            raise ValueError("estimate_normals: the clouds of a list need one column count, dtype and device")
        if rows is not None:
            raise ValueError("estimate_normals: rows comes from the list itself")
        lens = [t.shape[0] for t in points]
        if max(lens) < 1:
            raise ValueError("estimate_normals: every cloud of the list is empty")
        batch = torch.nn.utils.rnn.pad_sequence(list(points), batch_first=True)
        rows = torch.tensor(lens, dtype=torch.int32)
    else:
        _check_points(points, "points")
        if points.dim() not in (2, 3):
            raise ValueError("estimate_normals: points must be (m, c) or (N, m, c), got shape %s" % (tuple(points.shape),))
        batch = points if points.dim() == 3 else points.unsqueeze(0)
    N, m, c = batch.shape
    if N < 1 or m < 1:
        raise ValueError("estimate_normals: empty batch, shape %s" % (tuple(batch.shape),))
    if rows is not None:
        r = torch.as_tensor(rows)
        if r.dtype.is_floating_point or r.dtype == torch.bool or r.numel() != N:
            raise ValueError("estimate_normals: rows must be %d integer counts" % N)
        if not r.is_cuda:
            host = r.reshape(-1)
            if int(host.min()) < 0 or int(host.max()) > m:
                raise ValueError("estimate_normals: rows must lie in [0, %d]" % m)
    vp = None
    if viewpoint is not None:
        vp = torch.as_tensor(viewpoint)
        if vp.dtype.is_complex or vp.dtype == torch.bool or vp.shape not in ((3,), (N, 3)):
            raise ValueError("estimate_normals: viewpoint must be (3,) or (%d, 3), got shape %s" % (N, tuple(vp.shape)))

    on_cpu = not batch.is_cuda
    dev = compute_device() if on_cpu else batch.device
    x = batch.to(dev).contiguous()
    rows_d = torch.as_tensor(rows).to(device=dev, dtype=torch.int32).reshape(-1).contiguous() if rows is not None else None
    vp_d = vp.detach().to(device=dev, dtype=x.dtype).contiguous() if vp is not None else None
    nrm, curv, nbr = _Normals.apply(x, rows_d, vp_d, k, bool(return_neighbors))
    outs = [nrm] + ([curv] if return_curvature else []) + ([nbr] if return_neighbors else [])
    if on_cpu:
        outs = [o.cpu() for o in outs]
    if is_list:
        outs = [[o[b, :lens[b]] for b in range(N)] for o in outs]
    elif points.dim() == 2:
        outs = [o[0] for o in outs]
    return outs[0] if len(outs) == 1 else tuple(outs)
