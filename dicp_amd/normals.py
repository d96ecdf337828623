"""Differentiable surface normals for point-to-plane targets.

`ICP(icp_type='pt2pl')` takes target rows (m, 6) = xyz + unit normal.  `estimate_normals` computes those normals from the points
alone, on the GPU (libdicp_hip.so: dicp_normals_forward / dicp_normals_backward, or dicp_normals_grid_forward / dicp_normals_grid_backward
with method="grid"), with gradients back to the points -- summed with float atomics, or with deterministic=True stored once per element
from the inverted index of the neighbours (dicp_normals_backward_records / dicp_normals_gather_det):

    from dicp_amd.normals import estimate_normals
    nrm = estimate_normals(pts, k=16)
    target = torch.cat((pts, nrm), dim=-1)        # -> ICP(icp_type='pt2pl').icp(source, target, ...)

`estimate_normals_ball` takes EVERY row of a ball of radius R instead of the k <= 32 nearest rows -- the neighbourhood of
iss_keypoints_ball and fpfh_features_ball (dicp_normals_ball_forward / _records / _gather; the rules: csrc/dicp_normals_ball.h) -- and its
gradient is a gather over each row's own ball walk: no index, no atomics, bit-reproducible with no switch.
"""

import numbers

import torch

from . import _clouds, _lib
from ._clouds import ROW, _check_method
from ._ops import _DT, _p, _workspace
from .group import _invert
from .iss import _ball_grid, _check_ball_radius, _check_flag

REC = 13                # NRM_REC (csrc/dicp_normals_det.h): the doubles of a row's record, G6[0:6], mu[6:9], p[9:12], f[12]

K_MIN, K_MAX = 3, 32


class _Normals(torch.autograd.Function):
    """(N,m,c) points -> (normals (N,m,3), curvature (N,m), neighbours (N,m,k) int64 or None): one library call per direction on the current
    stream, into one allocation per direction.  grid: the neighbours from the cloud's cell grid (dicp_normals_grid_*) instead of the
    x-sorted walk; visited / passes: its optional (N,) int64 counters.  det: the backward stores every element once (_backward_det); records:
    an optional list that backward appends its (records, nbr_o) to."""

    @staticmethod
    def forward(ctx, pts, rows, vp, k, want_nbr, grid, visited, passes, det, records):
        N, m, c = pts.shape
        dt = _DT[pts.dtype]
        lib = _lib.load()
        ts = pts.element_size()
        ws_bytes = (lib.dicp_normals_grid_workspace_bytes if grid else lib.dicp_normals_workspace_bytes)(dt, N, m, k, c, 0)
        up = lambda x: (x + 255) // 256 * 256
        o_nrm, o_curv = 0, up(N * m * 3 * ts)
        o_nbr = o_curv + up(N * m * ts)
        o_ws = o_nbr + (up(N * m * k * 8) if want_nbr else 0)
        buf = _workspace(o_ws + ws_bytes, pts.device)
        nrm = buf[o_nrm: o_nrm + N * m * 3 * ts].view(pts.dtype).view(N, m, 3)
        curv = buf[o_curv: o_curv + N * m * ts].view(pts.dtype).view(N, m)
        nbr = buf[o_nbr: o_nbr + N * m * k * 8].view(torch.int64).view(N, m, k) if want_nbr else None
        ws = buf[o_ws:]
        per_cloud = int(vp is not None and vp.dim() == 2)
        counters = (_p(visited), _p(passes)) if grid else (None,)        # (the walk's `walked` counter is not asked for)
        _lib.call("dicp_normals_grid_forward" if grid else "dicp_normals_forward", pts.device, dt, _p(pts), c, _p(rows), N, m, k, _p(vp), per_cloud,
                  _p(nrm), _p(curv), _p(nbr), _p(ws), ws_bytes, *counters)
        ctx.save_for_backward(rows, vp)
        ctx.ws = ws                                     # (a view of the outputs' allocation: kept off the saved-tensor version checks)
        ctx.shape, ctx.k, ctx.grid, ctx.det, ctx.records = (N, m, c), k, grid, det, records
        ctx.set_materialize_grads(False)
        if nbr is not None:
            ctx.mark_non_differentiable(nbr)
        return nrm, curv, nbr

    @staticmethod
    def backward(ctx, g_nrm, g_curv, _g_nbr):
        if g_nrm is None and g_curv is None:
            return (None,) * 10
        rows, vp = ctx.saved_tensors
        ws = ctx.ws
        N, m, c = ctx.shape
        dtype = g_nrm.dtype if g_nrm is not None else g_curv.dtype
        dt = _DT[dtype]
        if ctx.det:
            return (_backward_det(ctx, g_nrm, g_curv, rows, vp, dtype),) + (None,) * 9
        lib = _lib.load()
        ts = torch.empty((), dtype=dtype).element_size()
        g_bytes = (lib.dicp_normals_grid_workspace_bytes if ctx.grid else lib.dicp_normals_workspace_bytes)(dt, N, m, ctx.k, c, 1)
        o_gws = (N * m * c * ts + 255) // 256 * 256
        buf = _workspace(o_gws + g_bytes, ws.device)
        grad = buf[:N * m * c * ts].view(dtype).view(N, m, c)
        gws = buf[o_gws:]
        g_nrm = g_nrm.contiguous() if g_nrm is not None else None
        g_curv = g_curv.contiguous() if g_curv is not None else None
        per_cloud = int(vp is not None and vp.dim() == 2)
        if ctx.grid:
            _lib.call("dicp_normals_grid_backward", ws.device, dt, _p(g_nrm), _p(g_curv), _p(vp), per_cloud, N, m, ctx.k, c,
                      _p(ws), _p(grad), _p(gws), gws.numel())
        else:
            _lib.call("dicp_normals_backward", ws.device, dt, _p(g_nrm), _p(g_curv), _p(vp), per_cloud, _p(rows), N, m, ctx.k, c,
                      _p(ws), _p(grad), _p(gws), gws.numel())
        return (grad,) + (None,) * 9


def _backward_det(ctx, g_nrm, g_curv, rows, vp, dtype):
    """The points' gradient with deterministic=True -> (N,m,c): the records pass (every query's G6, mu, p, f and its neighbours as original
    rows, at its original row), the inverted index of those neighbours -- built here, once, and only because the points need a gradient
    -- and the gather, which stores every element once.  Allocations and launches on the current stream only."""
    ws = ctx.ws
    N, m, c = ctx.shape
    dt = _DT[dtype]
    g_nrm = g_nrm.contiguous() if g_nrm is not None else None
    g_curv = g_curv.contiguous() if g_curv is not None else None
    records = torch.empty((N, m, REC), dtype=torch.float64, device=ws.device)
    nbr_o = torch.empty((N, m, ctx.k), dtype=torch.int32, device=ws.device)
    _lib.call("dicp_normals_backward_records", ws.device, dt, int(ctx.grid), _p(g_nrm), _p(g_curv), _p(vp), int(vp is not None and vp.dim() == 2),
              _p(rows), N, m, ctx.k, c, _p(ws), ws.numel(), _p(records), _p(nbr_o))
    off, slots = _invert(nbr_o, rows, m)
    grad = torch.empty((N, m, c), dtype=dtype, device=ws.device)
    _lib.call("dicp_normals_gather_det", ws.device, dt, _p(records), _p(nbr_o), 0, _p(rows), N, m, ctx.k, c, _p(off), _p(slots), _p(grad))
    if ctx.records is not None:
        ctx.records.append((records, nbr_o))
    return grad


def estimate_normals(points, k=16, viewpoint=None, rows=None, return_curvature=False, return_neighbors=False, method="walk",
                     deterministic=False, _visited=None, _passes=None, _records=None):
    """Unit surface normals of every point from its k nearest neighbours in its own cloud.

    points: (m, c), (N, m, c) with c >= 3 (columns 0:3 are used), or a list of (m_b, c); float32 or float64.  CPU tensors are computed on the
        GPU and returned on the CPU.
    k: 3 <= k <= 32.  rows: optional (N,) row counts of a padded batch (as ICP.icp's target_rows); rows past them are padding.
    viewpoint: None (the origin, as for a scan in its sensor frame), (3,) or (N, 3): each normal is flipped to face it.
    method: "walk" (the default) searches the neighbours along the x-sorted cloud; "grid" sorts the cloud into a cell grid whose cell edge is
        chosen on the device from the cloud's own density (as knn_points(method="grid"); the proof is csrc/dicp_gridknn.h) and lets every
        point grow a box of cells until its k-th distance is proved final.  Both are exact: on every cloud the walk defines -- all rows
        below the row count finite, no d2 that overflows -- they return the same neighbour lists and the same bits of normals and
        curvature, and differ in speed only (README, "Surface normals").  Where the walk leaves its output unspecified, "grid" follows
        knn_points' rule: the candidates of point i are the rows below the row count with three finite coordinates whose d2 to i is
        finite, and k_eff(i) = min(k, their number); a row with a non-finite coordinate is nobody's neighbour and gets a zero normal,
        zero curvature, -1 neighbours and no gradient; k_eff(i) < 3 gives the zero normal.  Nothing is read back from the device.
    deterministic: a bool (anything else is a ValueError before any device work); see "Gradients".

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
    points there; so does a point with k_eff < 3 or whose cotangents are all zero.  By default the terms are added with float atomics, and
    the last bits can differ from run to run.  With deterministic=True the forward is the default call's, bit for bit, and row j receives,
    per component, the sum over its list in the inverted index of the neighbour tensor (group.invert_neighbors(nbr, m, rows=rows): the
    slots q = i k + o with nbr[i, o] = j, in ascending q; built once inside the backward and only when the points need a gradient) of
    t_a = (T)(f ((G_a0 d_0 + G_a1 d_1) + G_a2 d_2)), d_c = ((double)y_c - (double)p_c) - mu_c, f = 2 / k_eff, with y row j's coordinates
    and p, mu, G = dL/dC query i's: one rounding per operation in double, one to the points' dtype T.  An entry whose query contributes
    nothing has no term; its position still counts.  The list is summed in chunks of group.DET_CHUNK = 64 positions, each from +0 by plain
    additions in T, the partials added in order to a total that starts at +0, a list of at most one chunk giving its partial itself.
    Every element is stored exactly once (no zero fill, no atomics): the result is bit-reproducible, the same bytes under "walk" and
    "grid" wherever the walk is defined, and within rounding of the default's (a term may differ from the atomic path's in the last bit
    of the double before it is rounded to T).
    """
    _clouds._check_k(k, "estimate_normals", K_MIN, K_MAX)
    _check_method(method, "estimate_normals")
    _clouds._check_deterministic(deterministic, "estimate_normals")
    form, batch, rows, lens = _clouds.check(points, rows, "estimate_normals", flat_rows=True)
    N, m = batch.shape[0], batch.shape[1]
    vp = None
    if viewpoint is not None:
        vp = torch.as_tensor(viewpoint)
        if vp.dtype.is_complex or vp.dtype == torch.bool or vp.shape not in ((3,), (N, 3)):
            raise ValueError("estimate_normals: viewpoint must be (3,) or (%d, 3), got shape %s" % (N, tuple(vp.shape)))

    on_cpu, x, rows_d = _clouds.place(batch, rows)
    vp_d = vp.detach().to(device=x.device, dtype=x.dtype).contiguous() if vp is not None else None
    nrm, curv, nbr = _Normals.apply(x, rows_d, vp_d, k, bool(return_neighbors), method == "grid", _visited, _passes, deterministic, _records)
    outs = [(ROW, nrm)] + ([(ROW, curv)] if return_curvature else []) + ([(ROW, nbr)] if return_neighbors else [])
    outs = _clouds.restore(form, on_cpu, m, lens, outs)
    return outs[0] if len(outs) == 1 else outs


# ------------------------------------------------------------------ the whole-ball form
class _NormalsBall(torch.autograd.Function):
    """(N,m,c) points -> (normals (N,m,3), curvature (N,m), eigenvalues (N,m,3), counts (N,m) int32): one grid build and one launch on the
    current stream; the backward is two launches (records, gather) on the grid and the state the forward kept.  visited: optional
    ((N,), (N,)) int64 counters of the forward's and the gather's walks; records: an optional list that backward appends its records to."""

    @staticmethod
    def forward(ctx, pts, rows, vp, radius, min_nb, visited, records):
        N, m, c = pts.shape
        dev = pts.device
        dt = _DT[pts.dtype]
        ws_bytes = _lib.load().dicp_normals_ball_workspace_bytes(N, m)
        if ws_bytes == 0:
            raise ValueError("estimate_normals_ball: N * m must stay below 2^31, got N = %d, m = %d" % (N, m))
        grid = _ball_grid(pts, rows, radius)
        ws = _workspace(ws_bytes, dev)
        nrm = torch.empty((N, m, 3), dtype=pts.dtype, device=dev)
        curv = torch.empty((N, m), dtype=pts.dtype, device=dev)
        eig = torch.empty((N, m, 3), dtype=pts.dtype, device=dev)
        cnt = torch.empty((N, m), dtype=torch.int32, device=dev)
        _lib.call("dicp_normals_ball_forward", dev, dt, _p(grid.plans), _p(grid.keys), _p(grid.perm), _p(grid.rows4), N, m, radius, min_nb, _p(vp),
                  int(vp is not None and vp.dim() == 2), _p(ws), ws_bytes, _p(nrm), _p(curv), _p(eig), _p(cnt),
                  _p(visited[0]) if visited is not None else None)
        ctx.grid, ctx.ws, ctx.ws_bytes = grid, ws, ws_bytes         # (kept off the saved-tensor version checks, as _Normals keeps ctx.ws)
        ctx.shape, ctx.radius, ctx.visited, ctx.records = (N, m, c), radius, visited, records
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(eig, cnt)
        return nrm, curv, eig, cnt

    @staticmethod
    def backward(ctx, g_nrm, g_curv, _g_eig, _g_cnt):
        if g_nrm is None and g_curv is None:
            return (None,) * 7
        grid, ws = ctx.grid, ctx.ws
        N, m, c = ctx.shape
        dev = ws.device
        dtype = g_nrm.dtype if g_nrm is not None else g_curv.dtype
        dt = _DT[dtype]
        g_nrm = g_nrm.contiguous() if g_nrm is not None else None
        g_curv = g_curv.contiguous() if g_curv is not None else None
        rec = torch.empty((N, grid.slots, REC), dtype=torch.float64, device=dev)
        _lib.call("dicp_normals_ball_records", dev, dt, _p(grid.plans), _p(grid.perm), _p(grid.rows4), N, m, _p(g_nrm), _p(g_curv), _p(ws), ctx.ws_bytes,
                  _p(rec))
        grad = torch.empty((N, m, c), dtype=dtype, device=dev)
        _lib.call("dicp_normals_ball_gather", dev, dt, _p(grid.plans), _p(grid.keys), _p(grid.perm), _p(grid.rows4), N, m, c, ctx.radius, _p(rec),
                  _p(grad), _p(ctx.visited[1]) if ctx.visited is not None else None)
        if ctx.records is not None:
            ctx.records.append((rec, grid))
        return (grad,) + (None,) * 6


def estimate_normals_ball(points, radius, viewpoint=None, rows=None, min_neighbors=3, return_curvature=False, return_eigenvalues=False,
                          return_counts=False, _visited=None, _records=None):
    """Unit surface normals of every point from EVERY row of its ball of radius `radius`: Open3D's estimate_normals with a radius search,
    over the same support as iss_keypoints_ball and fpfh_features_ball at that radius.

    points, rows, viewpoint: exactly as estimate_normals.  radius: required, a finite Python float > 0 whose square is finite.
    min_neighbors: an int >= 3; it counts the row itself.  The flags are bools.  Anything else is a ValueError before any device work.

    Definition (csrc/dicp_normals_ball.h; tests/normals_ball_ref.py is its numpy restatement), in double on the exactly converted inputs.
    The members of a row, their order, the mean and the covariance are iss_saliency_ball's, bit for bit: the row itself, then all other
    live rows (j < rows[b], three finite coordinates) with (dx dx + dy dy) + dz dz <= radius radius, in ascending (cell key, row index)
    order of the cloud's cell grid at the radius rounded UP to the points' dtype; two walks, never raw second moments.  The eigen-system
    is that pass's cyclic Jacobi with the rotations also applied to a matrix of eigenvectors, so the eigenvalues equal
    iss_saliency_ball(return_eigenvalues=True)'s bits.  n = s v_0 with s = +-1 so that n . (viewpoint - p_i) >= 0 (on exactly 0: the
    first non-zero component positive); curvature = lam_0 / ((lam_0 + lam_1) + lam_2), 0 unless the trace is > 0.  A row that is not
    live gets a zero normal, curvature 0, eigenvalues 0, count 0 and no gradient; a live row with fewer than min_neighbors members a zero
    normal and curvature 0, its count and eigenvalues are still reported.

    Returns normals (..., m, 3) in the points' dtype (a list for a list); with the flags, in this order, also curvature (..., m),
    eigenvalues (..., m, 3) ascending and counts (..., m) int32.

    Gradients flow to points[..., :3] (zero for the other columns); the viewpoint, the membership and the sign get none.  A row whose two
    smallest eigenvalues are not separated (lam_1 - lam_0 <= tau trace, tau = 1e-6 for float32 and 1e-12 for float64, as estimate_normals),
    with fewer than min_neighbors members, a zero trace or all-zero cotangents contributes nothing (it still receives the terms of the
    members whose balls hold it: their normals depend on it).  Ball membership is symmetric -- the double r2 of (i, j) and of (j, i)
    are the same bits -- so the gradient of row j is a GATHER over j's own ball walk: the sum over its
    members i, in j's member order (j first), of f_i ((G_a0 d_0 + G_a1 d_1) + G_a2 d_2), d = (p_j - p_i) - mu_i, f_i = 2 / n_i, G = dL/dC of
    row i, in double from +0, rounded once to the points' dtype.  No neighbour index, no inverted index, no float atomics, no zero fill:
    every element is stored exactly once and the result is bit-reproducible by construction.

    One grid build and one launch per call on the current stream (the backward: two launches, one of them a walk); no index or distance
    tensor exists at any point and nothing is read back, so a call on device tensors with device rows or no rows can sit in a captured
    graph, forward and backward.  A lane tests every row of the cells that can hold a member: the cost follows the rows visited.
    """
    what = "estimate_normals_ball"
    for name, flag in (("return_curvature", return_curvature), ("return_eigenvalues", return_eigenvalues), ("return_counts", return_counts)):
        _check_flag(flag, what, name)
    r = _check_ball_radius(radius, what, "radius")
    if isinstance(min_neighbors, bool) or not isinstance(min_neighbors, numbers.Integral) or min_neighbors < 3 or min_neighbors > 2 ** 31 - 1:
        raise ValueError("%s: min_neighbors must be an int >= 3, got %r" % (what, min_neighbors))
    form, batch, rows, lens = _clouds.check(points, rows, what, flat_rows=True)
    N, m = batch.shape[0], batch.shape[1]
    vp = None
    if viewpoint is not None:
        vp = torch.as_tensor(viewpoint)
        if vp.dtype.is_complex or vp.dtype == torch.bool or vp.shape not in ((3,), (N, 3)):
            raise ValueError("%s: viewpoint must be (3,) or (%d, 3), got shape %s" % (what, N, tuple(vp.shape)))
    on_cpu, x, rows_d = _clouds.place(batch, rows)
    vp_d = vp.detach().to(device=x.device, dtype=x.dtype).contiguous() if vp is not None else None
    nrm, curv, eig, cnt = _NormalsBall.apply(x, rows_d, vp_d, r, int(min_neighbors), _visited, _records)
    outs = [(ROW, nrm)] + [(ROW, t) for t, on in ((curv, return_curvature), (eig, return_eigenvalues), (cnt, return_counts)) if on]
    outs = _clouds.restore(form, on_cpu, m, lens, outs)
    return outs[0] if len(outs) == 1 else outs
