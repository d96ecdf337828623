"""ISS keypoints (Intrinsic Shape Signatures, Zhong 2009, in the form of Open3D's ComputeISSKeypoints) from points and neighbours.

The keypoint stage of a classical global registration, on the GPU (libdicp_hip.so: dicp_iss_saliency / dicp_iss_maxima; the rules:
csrc/dicp_iss.h).  Descriptors are matched and pruned on a few hundred well-spread, repeatable points instead of on every point:

    from dicp_amd.iss import compute_iss_keypoints
    fx, fy = compute_fpfh(x, nx, 0.8), compute_fpfh(y, ny, 0.8)                # descriptors of every point, as before
    kx, rows_x, ix = compute_iss_keypoints(x, 0.6, return_index=True)          # ix: the rows of x that are keypoints
    ky, rows_y, iy = compute_iss_keypoints(y, 0.6, return_index=True)
    idx, _ = match_features(fx[ix], fy[iy], mutual=True)                       # (or select_rows of the descriptors with the same mask)
    T0, inliers = ransac_correspondences(kx, ky, idx, 0.1)                     # -> ICP(...).icp(x, y, T_init=T0)

Limits.  In the k-slot form (iss_saliency / iss_keypoints / compute_iss_keypoints by default) a neighbourhood is at most the k <= 32
NEAREST rows of the ball plus the row itself, where Open3D uses every row of the ball: choose the radius for the voxel size so that a ball
holds about that many, and idx comes from ball_query or knn_points (no search fused into those passes).  The whole-ball form
(iss_saliency_ball / iss_keypoints_ball / compute_iss_keypoints(whole_ball=True); libdicp_hip.so: dicp_iss_ball_saliency /
dicp_iss_ball_maxima, the member list: csrc/dicp_iss_ball.h) has no such limit: it walks every row of the ball on the cloud's cell grid
and takes no index.  Its sums run over the members in cell order, so its eigenvalues differ from the k-slot form's in the last bits
even where both see the same members.  No gradients in either form: the outputs are decisions (the kept rows of compute_iss_keypoints get
theirs through select_rows).
"""
import math
import numbers

import torch

from . import _clouds, _lib
from ._clouds import ROW
from ._grid import CellGrid
from ._ops import _DT, _p, _workspace
from .ball import ball_query
from .filter import select_rows
from .fpfh import _check_radius

K_MIN, K_MAX = 1, 32                # ISS_K_MIN, ISS_K_MAX (csrc/dicp_iss.h): the slots of idx


def _check_gamma(g, what, name):
    ok = not isinstance(g, bool) and isinstance(g, (int, float))
    if ok:
        g = float(g)
        ok = 0.0 < g <= 1.0                                 # (a NaN fails both)
    if not ok:
        raise ValueError("%s: %s must be a float in (0, 1], got %r" % (what, name, g))
    return g


def _check_min_neighbors(n, what):
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1 or n > 2 ** 31 - 1:
        raise ValueError("%s: min_neighbors must be an int >= 1, got %r" % (what, n))
    return int(n)


def _check_flag(v, what, name):
    if not isinstance(v, bool):
        raise ValueError("%s: %s must be True or False, got %r" % (what, name, v))


def _check_idx(idx, what, name, form, batch, lens):
    ib, ilens = _clouds.check_slots(idx, what, name, (form, batch), True, K_MIN, K_MAX)
    if ib.shape[1] != batch.shape[1] or (lens is not None and list(ilens) != list(lens)):
        raise ValueError("%s: %s must be a search of the cloud against itself, one row of slots per point: got %s rows for %s points"
                         % (what, name, ilens if lens is not None else ib.shape[1], lens if lens is not None else batch.shape[1]))
    return ib


def _saliency(x, idx, rows_d, radius, g21, g32, min_nb, want_eig, want_cnt):
    """placed arguments -> (ws, ws_bytes, saliency (N,m), eigenvalues (N,m,3) or None, counts (N,m) int32 or None): one launch"""
    N, m, c = x.shape
    dev = x.device
    ws_bytes = _lib.load().dicp_iss_workspace_bytes(N, m)
    if ws_bytes == 0:
        raise ValueError("iss_saliency: N * m must stay below 2^31, got N = %d, m = %d" % (N, m))
    ws = _workspace(ws_bytes, dev)
    sal = torch.empty((N, m), dtype=x.dtype, device=dev)
    eig = torch.empty((N, m, 3), dtype=x.dtype, device=dev) if want_eig else None
    cnt = torch.empty((N, m), dtype=torch.int32, device=dev) if want_cnt else None
    _lib.call("dicp_iss_saliency", dev, _DT[x.dtype], _p(x), c, _p(idx), 1 if idx.dtype == torch.int64 else 0, _p(rows_d), N, m, idx.shape[2],
              radius, g21, g32, min_nb, _p(ws), ws_bytes, _p(sal), _p(eig), _p(cnt))
    return ws, ws_bytes, sal, eig, cnt


def _maxima(x, idx, rows_d, radius, min_nb, ws, ws_bytes):
    """the keypoint mask (N,m) bool from the workspace _saliency left: one launch"""
    N, m, c = x.shape
    mask = torch.empty((N, m), dtype=torch.bool, device=x.device)
    _lib.call("dicp_iss_maxima", x.device, _DT[x.dtype], _p(x), c, _p(idx), 1 if idx.dtype == torch.int64 else 0, _p(rows_d), N, m, idx.shape[2],
              radius, min_nb, _p(ws), ws_bytes, _p(mask))
    return mask


def iss_saliency(points, idx, rows=None, radius=None, gamma21=0.975, gamma32=0.975, min_neighbors=5, return_eigenvalues=False,
                 return_counts=False):
    """The ISS saliency of every point -- the smallest eigenvalue of its neighbourhood's covariance where the three eigenvalues are
    well separated, 0 elsewhere -- on the GPU.

    points: (m, c), (N, m, c) or a list of (m_b, c) with c >= 3; float32 or float64; columns 0:3 are the coordinates, the others are not
        read.  CPU tensors are computed on the GPU and returned on the CPU.
    idx: the neighbours of every point IN ITS OWN CLOUD -- the idx of ball_query(p, p, ...) or knn_points(p, p, ...): (m, k), (N, m, k) or a
        list of (m_b, k), int64 or int32, 1 <= k <= 32, on the points' device.  A slot is empty when its index is negative or at or past
        the cloud's row count; the row itself is skipped wherever it stands.  The kernels never read out of range whatever idx holds.
    rows: optional (N,) row counts of a padded batch.
    radius: None, or a finite Python float > 0: slots whose r2, RECOMPUTED here in double, exceeds radius * radius are dropped.
    gamma21, gamma32: floats in (0, 1].  min_neighbors: an int >= 1; the row counts itself.
    Anything else is a ValueError before any device work.

    Definition (csrc/dicp_iss.h states every operation; tests/iss_ref.py is its numpy restatement).  All arithmetic is in double on the
    exactly converted inputs, with + - * / sqrt only.  A row is OK when its coordinates are finite.  The members of row i are the row
    itself, then in slot order the slots naming another OK row of the cloud within the radius (duplicates at distance 0 included);
    count is their number.  Over the members: q = p_j - p_i, mu = sum(q) / count, the covariance sum((q - mu)(q - mu)^T) / count, its
    eigenvalues l0 <= l1 <= l2 by six cyclic Jacobi sweeps.  saliency = l0 when count >= min_neighbors, l1 < gamma21 l2 and
    0 < l0 < gamma32 l1 (Open3D's rule, written with products), else 0.  Rows that are not OK, and rows at or past rows[b], get zeros.

    Returns the saliency (m,) / (N, m) / a list of (m_b,) in the points' dtype, rounded once; with return_eigenvalues=True also the
    eigenvalues (..., 3) ascending in the points' dtype (on their own: linearity (l2 - l1) / l2, planarity (l1 - l0) / l2, scattering
    l0 / l2), with return_counts=True also the int32 counts -- as a tuple (saliency[, eigenvalues][, counts]).

    Limits: a neighbourhood is at most the k <= 32 slots of idx plus the row itself (Open3D uses every row of the ball).  No gradients:
    the outputs never require grad.  No fused search.  Nothing is read back and the launch is on the current stream: a call on device
    tensors with device (or no) rows can sit in a captured graph.  No float atomics: the result is bit-reproducible.
    """
    what = "iss_saliency"
    _check_flag(return_eigenvalues, what, "return_eigenvalues")
    _check_flag(return_counts, what, "return_counts")
    radius = _check_radius(radius, what)
    g21, g32 = _check_gamma(gamma21, what, "gamma21"), _check_gamma(gamma32, what, "gamma32")
    min_nb = _check_min_neighbors(min_neighbors, what)
    form, batch, rows, lens = _clouds.check(points, rows, what)
    ib = _check_idx(idx, what, "idx", form, batch, lens)
    on_cpu, x, rows_d = _clouds.place(batch, rows)
    _, _, sal, eig, cnt = _saliency(x.detach(), ib.to(x.device).contiguous(), rows_d, radius, g21, g32, min_nb, return_eigenvalues, return_counts)
    outs = _clouds.restore(form, on_cpu, batch.shape[1], lens, [(ROW, t) for t in (sal, eig, cnt) if t is not None])
    return outs if len(outs) > 1 else outs[0]


def iss_keypoints(points, idx, rows=None, salient_radius=None, non_max_radius=None, gamma21=0.975, gamma32=0.975, min_neighbors=5, nms_idx=None,
                  return_saliency=False):
    """The ISS keypoints of every cloud as a torch.bool mask, ready for select_rows: iss_saliency, then a non-maximum suppression.

    points, idx, rows, gamma21, gamma32, min_neighbors: as iss_saliency.  salient_radius: the radius of the saliency pass;
    non_max_radius: the radius of the suppression (each None or a finite Python float > 0, each on its own: None is no cut).
    nms_idx: an optional second self index, in the form of idx (its k may differ), for the suppression; by default idx itself serves
    both passes under the two radii.

    Row i is a keypoint when saliency_i > 0, its member count for the suppression's index and radius is at least min_neighbors, and no
    member j has saliency_j > saliency_i, or saliency_j == saliency_i and j < i.  The tie rule is the one departure from Open3D, which
    keeps both sides of an exact tie: exact duplicates yield one keypoint, the lower row.  The comparison is on the double saliencies of
    the first pass, never on a rounded output.

    Returns the mask (m,) / (N, m) / a list of (m_b,); with return_saliency=True (mask, saliency).  Two launches on the current stream,
    nothing read back; no gradients.  The limits are iss_saliency's.
    """
    what = "iss_keypoints"
    _check_flag(return_saliency, what, "return_saliency")
    r1, r2 = _check_radius(salient_radius, what), _check_radius(non_max_radius, what)
    g21, g32 = _check_gamma(gamma21, what, "gamma21"), _check_gamma(gamma32, what, "gamma32")
    min_nb = _check_min_neighbors(min_neighbors, what)
    form, batch, rows, lens = _clouds.check(points, rows, what)
    ib = _check_idx(idx, what, "idx", form, batch, lens)
    nb = ib if nms_idx is None else _check_idx(nms_idx, what, "nms_idx", form, batch, lens)
    on_cpu, x, rows_d = _clouds.place(batch, rows)
    xd = x.detach()
    i1 = ib.to(x.device).contiguous()
    i2 = i1 if nms_idx is None else nb.to(x.device).contiguous()
    ws, ws_bytes, sal, _, _ = _saliency(xd, i1, rows_d, r1, g21, g32, min_nb, False, False)
    mask = _maxima(xd, i2, rows_d, r2, min_nb, ws, ws_bytes)
    outs = _clouds.restore(form, on_cpu, batch.shape[1], lens, [(ROW, mask)] + ([(ROW, sal)] if return_saliency else []))
    return outs if return_saliency else outs[0]


# ------------------------------------------------------------------ the whole-ball form
def _check_ball_radius(radius, what, name):
    """a finite Python float > 0 whose square is finite -> the float"""
    r = None if radius is None else _check_radius(radius, what)
    if r is None or not math.isfinite(r * r):
        raise ValueError("%s: %s must be a finite float > 0 with a finite square, got %r" % (what, name, radius))
    return r


def _grid_radius(r, dtype):
    """The smallest number of dtype that is not below the Python float r, the largest finite one where that would be infinite
    (csrc/dicp_iss_ball.h: iss_ball_grid_radius): a float32 conversion can round DOWN, and the grid's cells must not be cut for less
    than the radius asked for.  Host arithmetic on a 0-d CPU tensor: no device work."""
    if dtype == torch.float64:
        return r
    big = torch.finfo(torch.float32).max
    if r >= big:
        return big
    t = torch.tensor(r, dtype=torch.float32)
    if float(t) < r:
        t = torch.nextafter(t, torch.tensor(math.inf, dtype=torch.float32))
    return float(t)


def _ball_grid(x, rows_d, radius):
    """the CellGrid of the placed batch x at the radius of a call, rounded up to x's dtype (filled on the device: no copy)"""
    return CellGrid(x, rows_d, torch.full((1,), _grid_radius(radius, x.dtype), dtype=x.dtype, device=x.device))


def _saliency_ball(grid, x, radius, g21, g32, min_nb, want_eig, want_cnt):
    """-> (ws, ws_bytes, saliency (N,m), eigenvalues (N,m,3) or None, counts (N,m) int32 or None): one launch on x's grid"""
    N, m, _ = x.shape
    dev = x.device
    ws_bytes = _lib.load().dicp_iss_workspace_bytes(N, m)
    if ws_bytes == 0:
        raise ValueError("iss_saliency_ball: N * m must stay below 2^31, got N = %d, m = %d" % (N, m))
    ws = _workspace(ws_bytes, dev)
    sal = torch.empty((N, m), dtype=x.dtype, device=dev)
    eig = torch.empty((N, m, 3), dtype=x.dtype, device=dev) if want_eig else None
    cnt = torch.empty((N, m), dtype=torch.int32, device=dev) if want_cnt else None
    _lib.call("dicp_iss_ball_saliency", dev, _DT[x.dtype], _p(grid.plans), _p(grid.keys), _p(grid.perm), _p(grid.rows4), N, m, radius, g21, g32,
              min_nb, _p(ws), ws_bytes, _p(sal), _p(eig), _p(cnt), None)
    return ws, ws_bytes, sal, eig, cnt


def iss_saliency_ball(points, radius, rows=None, gamma21=0.975, gamma32=0.975, min_neighbors=5, return_eigenvalues=False, return_counts=False):
    """The ISS saliency of every point over EVERY row of its ball, Open3D's neighbourhood: iss_saliency without an index and without its
    limit of 32 slots.

    points, rows, gamma21, gamma32, min_neighbors, the flags and the returns: as iss_saliency.  radius: required, a finite Python float
    > 0 whose square is finite.  Anything else is a ValueError before any device work.

    Definition (csrc/dicp_iss_ball.h; tests/iss_ball_ref.py is its numpy restatement).  Everything of iss_saliency stands; only the member
    list changes: the members of an OK row i are the row itself, then ALL other OK rows j < rows[b] of the cloud with
    (dx dx + dy dy) + dz dz <= radius radius in double on the exactly converted inputs (inclusive; duplicates at distance 0 included), in
    ascending (cell key, row index) order of the cloud's cell grid -- the grid ball_query builds (csrc/dicp_ball.h), at the radius
    rounded UP to the points' dtype: cell = floor((a - o) / s) per axis in the points' dtype with o the per-axis minimum of the OK rows and
    s = ball_R(that radius), keys compared as (cx, cy, cz).  A row is a member once; count includes the row itself.  The sums of the mean
    and of the covariance run over the members in that order (two walks: the mean first, never raw second moments).

    One grid build and one launch on the current stream; no index or distance tensor exists at any point.  A lane walks the cells that
    can hold a member (csrc/dicp_iss_ball.h proves that none is missed) and tests every row in them, so the cost follows the rows
    VISITED -- several times the members.  No gradients, nothing read back (a call on device tensors with device or no rows can sit in a
    captured graph), no float atomics: bit-reproducible.
    """
    what = "iss_saliency_ball"
    _check_flag(return_eigenvalues, what, "return_eigenvalues")
    _check_flag(return_counts, what, "return_counts")
    r = _check_ball_radius(radius, what, "radius")
    g21, g32 = _check_gamma(gamma21, what, "gamma21"), _check_gamma(gamma32, what, "gamma32")
    min_nb = _check_min_neighbors(min_neighbors, what)
    form, batch, rows, lens = _clouds.check(points, rows, what)
    on_cpu, x, rows_d = _clouds.place(batch, rows)
    xd = x.detach()
    _, _, sal, eig, cnt = _saliency_ball(_ball_grid(xd, rows_d, r), xd, r, g21, g32, min_nb, return_eigenvalues, return_counts)
    outs = _clouds.restore(form, on_cpu, batch.shape[1], lens, [(ROW, t) for t in (sal, eig, cnt) if t is not None])
    return outs if len(outs) > 1 else outs[0]


def iss_keypoints_ball(points, salient_radius, non_max_radius=None, rows=None, gamma21=0.975, gamma32=0.975, min_neighbors=5,
                       return_saliency=False):
    """The ISS keypoints of every cloud as a torch.bool mask over EVERY row of the two balls: iss_saliency_ball, then iss_keypoints' rule
    of suppression over all members within non_max_radius (None: the salient radius), on the double saliencies.

    ONE grid per call, built at the larger of the two radii; each pass enumerates the cells for its own radius.  The member ORDER of the
    saliency pass is that grid's: where non_max_radius is the larger, the saliencies can differ in their last bits from those of
    iss_saliency_ball(points, salient_radius), whose grid is built at the salient radius.  The suppression's walk
    stops at the first member that beats the row (the mask is then False whatever the count).  Returns as iss_keypoints; three steps on
    the current stream (grid, saliency, maxima), nothing read back; no gradients."""
    what = "iss_keypoints_ball"
    _check_flag(return_saliency, what, "return_saliency")
    r1 = _check_ball_radius(salient_radius, what, "salient_radius")
    r2 = r1 if non_max_radius is None else _check_ball_radius(non_max_radius, what, "non_max_radius")
    g21, g32 = _check_gamma(gamma21, what, "gamma21"), _check_gamma(gamma32, what, "gamma32")
    min_nb = _check_min_neighbors(min_neighbors, what)
    form, batch, rows, lens = _clouds.check(points, rows, what)
    on_cpu, x, rows_d = _clouds.place(batch, rows)
    xd = x.detach()
    N, m, _ = xd.shape
    grid = _ball_grid(xd, rows_d, max(r1, r2))
    ws, ws_bytes, sal, _, _ = _saliency_ball(grid, xd, r1, g21, g32, min_nb, False, False)
    mask = torch.empty((N, m), dtype=torch.bool, device=xd.device)
    _lib.call("dicp_iss_ball_maxima", xd.device, _DT[xd.dtype], _p(grid.plans), _p(grid.keys), _p(grid.perm), _p(grid.rows4), N, m, r2, min_nb,
              _p(ws), ws_bytes, _p(mask), None)
    outs = _clouds.restore(form, on_cpu, batch.shape[1], lens, [(ROW, mask)] + ([(ROW, sal)] if return_saliency else []))
    return outs if return_saliency else outs[0]


def compute_iss_keypoints(points, salient_radius, non_max_radius=None, k=32, rows=None, gamma21=0.975, gamma32=0.975, min_neighbors=5,
                          return_index=False, whole_ball=False):
    """The ISS keypoints of every cloud as points: one ball_query(points, points, max(salient_radius, non_max_radius), k) under no_grad,
    iss_keypoints on its idx with each pass cut by its own radius (ball_query keeps the NEAREST k, so the smaller ball's members are still
    its nearest), then select_rows(points, mask).  With whole_ball=True: iss_keypoints_ball (every row of the two balls, no index; k is
    checked but not used), then select_rows.

    points, rows, gamma21, gamma32, min_neighbors: as iss_saliency.  salient_radius: a finite Python float > 0; non_max_radius: the same,
    or None for the salient radius.  k: an int in [1, 32]; a point finds itself first, so k - 1 slots are left for its neighbours.
    whole_ball: True or False (anything else is a ValueError).

    Returns (keypoints, rows_out[, index]) as select_rows returns them: for a batch keypoints (N, m, c) zero-padded with all c columns,
    rows_out (N,) int32 and index (N, m) int64, the input row of every keypoint in order (-1 past rows_out).  The kept rows get their
    gradient through select_rows; the decision carries none.  The limits are iss_saliency's."""
    what = "compute_iss_keypoints"
    _check_flag(return_index, what, "return_index")
    _check_flag(whole_ball, what, "whole_ball")
    if salient_radius is None:
        raise ValueError("%s: salient_radius must be a finite float > 0, got None" % what)
    r1 = _check_radius(salient_radius, what)
    r2 = r1 if non_max_radius is None else _check_radius(non_max_radius, what)
    _check_gamma(gamma21, what, "gamma21")
    _check_gamma(gamma32, what, "gamma32")
    _check_min_neighbors(min_neighbors, what)
    _clouds._check_k(k, what, K_MIN, K_MAX)
    _clouds.check(points, rows, what)
    if whole_ball:
        _check_ball_radius(salient_radius, what, "salient_radius")
        _check_ball_radius(r2, what, "non_max_radius")
        with torch.no_grad():
            mask = iss_keypoints_ball(points, r1, r2, rows=rows, gamma21=gamma21, gamma32=gamma32, min_neighbors=min_neighbors)
        return select_rows(points, mask, rows=rows, return_index=return_index)
    with torch.no_grad():
        idx = ball_query(points, points, max(r1, r2), k=k, x_rows=rows, y_rows=rows)[1]
        mask = iss_keypoints(points, idx, rows=rows, salient_radius=r1, non_max_radius=r2, gamma21=gamma21, gamma32=gamma32,
                             min_neighbors=min_neighbors)
    return select_rows(points, mask, rows=rows, return_index=return_index)
