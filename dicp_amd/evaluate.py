"""How good is a pose?  Fitness, inlier RMSE and the 6x6 information matrix of candidate poses, many per cloud against one grid build.

Exact results on the GPU (libdicp_hip.so: dicp_ball_grid_build / dicp_evaluate_poses), without the (N, H, n) intermediates of a
composition of transform, ball_query and masked reductions:

    from dicp_amd.evaluate import evaluate_registration, information_matrix, best_pose
    fitness, rmse, counts = evaluate_registration(source, target, T, max_distance)
    info = information_matrix(source, target, T, max_distance)              # (..., 6, 6), a pose-graph edge's weight
    best, T_best = best_pose(T, counts, rmse)                               # the hypothesis to hand to ICP
"""
import math

import torch

from . import _clouds, _lib
from ._grid import CellGrid
from ._ops import _DT, _p
from .ball import _check_radius

H_MAX = 65536
TILE = 256              # source rows per workgroup (csrc/dicp_evaluate.h: EVAL_TILE)
# the slots of the kernel's sums (csrc/dicp_evaluate.h)
S_E, S_T, S_XX, S_YY, S_ZZ, S_XY, S_XZ, S_YZ = 0, 1, 4, 5, 6, 7, 8, 9


def _err(what, msg):
    raise ValueError("%s: %s" % (what, msg))


def _check_flag(v, name, what):
    if not isinstance(v, bool):
        _err(what, "%s must be True or False, got %r" % (name, v))


def _arguments(source, target, T, max_distance, source_rows, target_rows, what):
    """Every check, on the host -> (form, N, n, m, bs, rs, bt, rt, T (N,H,4,4), H, lead, radius): lead the leading shape of the outputs"""
    if isinstance(source, (list, tuple)) or isinstance(target, (list, tuple)):
        _err(what, "lists of clouds are not offered: pass single clouds (n, c) / (m, c) or padded batches with row counts")
    try:
        radius = _check_radius(max_distance)
    except ValueError as e:
        _err(what, "max_distance: %s" % str(e).split(": ", 1)[-1])
    (form, bs, rs, _), (_, bt, rt, _) = _clouds.check_pair(source, target, source_rows, target_rows, what, "source", "target")
    if isinstance(radius, float):
        r_t = float(torch.tensor(radius, dtype=bs.dtype))
        if not (math.isfinite(r_t) and r_t > 0.0):
            _err(what, "max_distance must be finite and > 0 in %s, got %r" % (bs.dtype, radius))
    N, n, m = bs.shape[0], bs.shape[1], bt.shape[1]
    if not isinstance(T, torch.Tensor):
        _err(what, "T must be a tensor, got %s" % type(T).__name__)
    if T.dtype != bs.dtype:
        _err(what, "T must have the dtype of the points, %s, got %s" % (bs.dtype, T.dtype))
    if T.device != bs.device:
        _err(what, "T and the points must be on one device, got %s and %s" % (T.device, bs.device))
    if T.dim() < 2 or tuple(T.shape[-2:]) != (4, 4):
        _err(what, "T must end in (4, 4), got shape %s" % (tuple(T.shape),))
    lead = tuple(T.shape[:-2])
    if form == "single":
        if len(lead) > 1:
            _err(what, "T must be (4, 4) or (H, 4, 4) for a single pair of clouds, got shape %s" % (tuple(T.shape),))
        H = lead[0] if lead else 1
    else:
        if len(lead) not in (1, 2) or lead[0] != N:
            _err(what, "T must be (N, 4, 4) or (N, H, 4, 4) with N = %d, got shape %s" % (N, tuple(T.shape)))
        H = lead[1] if len(lead) == 2 else 1
    if not (1 <= H <= H_MAX):
        _err(what, "the number of poses per cloud H must lie in [1, %d], got %d" % (H_MAX, H))
    if N * H * ((max(n, 1) + TILE - 1) // TILE) >= 2 ** 31:
        _err(what, "N H ceil(n / %d) = %d x %d x %d workgroups do not fit one launch (2^31)" % (TILE, N, H, (max(n, 1) + TILE - 1) // TILE))
    return form, N, n, m, bs, rs, bt, rt, T.detach().reshape(N, H, 4, 4), H, lead, radius


def _evaluate(source, target, T, max_distance, source_rows, target_rows, want_rows, what):
    """-> (on_cpu, n, lead, sums (N,H,10), counts (N,H), fitness (N,H), rmse (N,H), idx (N,H,n') or None, d2 or None)"""
    form, N, n, m, bs, rs, bt, rt, poses, H, lead, radius = _arguments(source, target, T, max_distance, source_rows, target_rows, what)
    on_cpu, src, srows = _clouds.place(bs.detach(), rs, xyz=True)
    _, tgt, trows = _clouds.place(bt.detach(), rt, xyz=True)
    dev, dt = src.device, src.dtype
    poses = poses.to(dev).contiguous()
    if isinstance(radius, torch.Tensor):
        r_d = radius.detach().to(device=dev, dtype=dt).reshape(1)
    else:
        r_d = torch.full((1,), radius, dtype=dt, device=dev)                     # (filled on the device, rounded to T: no copy)
    grid = CellGrid(tgt, trows, r_d)
    n_d, m_d = src.shape[1], tgt.shape[1]                                        # (>= 1: a cloud without rows is one pad row, count 0)
    ws_bytes = _lib.load().dicp_evaluate_workspace_bytes(N, H, n_d)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    sums = torch.empty((N, H, 10), dtype=torch.float64, device=dev)
    counts = torch.empty((N, H), dtype=torch.int32, device=dev)
    fitness = torch.empty((N, H), dtype=torch.float64, device=dev)
    rmse = torch.empty((N, H), dtype=torch.float64, device=dev)
    idx = torch.empty((N, H, n_d), dtype=torch.int64, device=dev) if want_rows else None
    d2 = torch.empty((N, H, n_d), dtype=dt, device=dev) if want_rows else None
    _lib.call("dicp_evaluate_poses", dev, _DT[dt], _p(src), src.shape[2], _p(srows), n_d, _p(poses), H, _p(grid.plans), _p(grid.keys), _p(grid.perm),
              _p(grid.rows4), m_d, N, _p(ws), ws_bytes, _p(sums), _p(counts), _p(fitness), _p(rmse), _p(idx), _p(d2))
    return on_cpu, n, lead, sums, counts, fitness, rmse, idx, d2


def _shaped(t, lead, on_cpu, tail=()):
    """(N, H, *tail) -> (*lead, *tail) on the caller's device"""
    t = t.reshape(tuple(lead) + tuple(tail))
    return t.cpu() if on_cpu else t


def evaluate_registration(source, target, T, max_distance, source_rows=None, target_rows=None, return_correspondences=False):
    """Fitness, inlier RMSE and inlier count of candidate poses: Open3D's evaluate_registration, for many poses per cloud at once.

    source, target: one cloud each, (n, c) and (m, c), or a padded batch each, (N, n, c) and (N, m, c), with optional integer row counts
        source_rows / target_rows (N,).  float32 or float64, one dtype and device; columns 0:3 are used.  Lists of clouds are not offered.
        CPU tensors are computed on the GPU and returned on the CPU.
    T: the poses that take source to target, in the points' dtype: (4, 4) or (H, 4, 4) for a single pair, (N, 4, 4) or (N, H, 4, 4) for a
        batch, H in [1, 65536]; rows 0:3 are read.  N H ceil(n / 256) must stay below 2^31.
    max_distance: exactly ball_query's radius -- a Python float or a 0-d tensor, finite and > 0; a 0-d tensor on the device is not read back.
    Anything malformed is a ValueError before any device work.

    Definition (hardware-independent; T below is the points' dtype, "double" means on exactly converted values with + - * / sqrt only and
    no fma):
      1 pose    of (cloud b, hypothesis h): C_ak = T[b,h,a,k], r_a = T[b,h,a,3].
      2 query   q_a = fma(C_a2, x_2, fma(C_a1, x_1, fma(C_a0, x_0, r_a))) in T, the chain of ransac_correspondences' rule 4.  Source row i
                is a QUERY under the pose when i < source_rows[b] and q_0, q_1, q_2 are finite.
      3 match   slot 0 of ball_query(q, target, max_distance, k=1, y_rows=target_rows), exactly: the candidates are the target rows
                j < target_rows[b] with finite coordinates and d2 = (dx dx + dy dy) + dz dz <= r2 (separate roundings in T, d = y_j - q),
                r2 = max_distance rounded to T, then squared in T; the winner is the first candidate in (d2, j) order.  Without a
                candidate idx = -1 and d2 = +inf.
      4 count   the number of matched queries; fitness = count / source_rows[b] in double (n without row counts), 0 for a cloud with
                no rows.
      5 terms   a matched row has ten double terms, with t = (double) y_match: e = (double) d2; t_x, t_y, t_z; t_x t_x, t_y t_y,
                t_z t_z, t_x t_y, t_x t_z, t_y t_z.  Every other row contributes +0 to each.
      6 order   of every sum, a function of n alone: tile c holds rows 256 c .. 256 c + 255 (rows at or past n contribute +0); within a
                tile v_l + v_(l + off) for off = 1, 2, 4, ..., 128 (the pairwise tree of gnc_correspondences' rule 2); the tile results
                are added in ascending c to a total that starts at +0.
      7 rmse    inlier_rmse = sqrt(SSE / count) in double, 0 when count = 0.
      8 matrix  information_matrix: Open3D's sum of G^T G over the matched TARGET points t, with the rows of G (0, z, -y, 1, 0, 0),
                (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1) -- rotation first --, assembled from the nine moment sums:
                L00 = Syy + Szz, L11 = Sxx + Szz, L22 = Sxx + Syy, L01 = -Sxy, L02 = -Sxz, L12 = -Syz,
                L[0:3, 3:6] = [[0, -Sz, Sy], [Sz, 0, -Sx], [-Sy, Sx, 0]], L[3:6, 3:6] = count I, L symmetric.  The sign of a zero entry
                is not part of the definition.
      9 best_pose: per cloud the hypothesis with the largest count, then the smallest rmse, then the lowest h.
    A non-finite pose, an empty target or a source with no rows gives count 0, fitness 0, rmse 0 and a zero matrix.

    Returns (fitness, inlier_rmse, counts): float64, float64 and int32 of shape (N, H), (N,), (H,) or 0-d, matching T; with
    return_correspondences=True also idx (..., n) int64 and d2 (..., n) in the points' dtype.  Nothing requires grad and the inputs are read
    detached: these are decisions and statistics (chamfer_distance is the differentiable objective).  Every output is bit-reproducible.

    The target is sorted into ONE cell grid per call (CellGrid, as ball_query), whatever H is; one workgroup takes 256 source rows of one
    (cloud, pose) in the original row order -- the queries are not re-sorted by cell, so a wave's locality is the caller's row order
    (voxel_downsample's output is in voxel order).  Nothing is read back from the device and no launch depends on device data: a call on
    device tensors can sit in a captured graph.
    """
    what = "evaluate_registration"
    _check_flag(return_correspondences, "return_correspondences", what)
    on_cpu, n, lead, _, counts, fitness, rmse, idx, d2 = _evaluate(source, target, T, max_distance, source_rows, target_rows, return_correspondences, what)
    out = (_shaped(fitness, lead, on_cpu), _shaped(rmse, lead, on_cpu), _shaped(counts, lead, on_cpu))
    if return_correspondences:
        out += (_shaped(idx[:, :, :n], lead, on_cpu, (n,)), _shaped(d2[:, :, :n], lead, on_cpu, (n,)))
    return out


def _assemble(sums, counts):
    """(..., 10) float64 sums and (...) counts -> (..., 6, 6) float64: rule 8"""
    S = sums
    L = torch.zeros(tuple(S.shape[:-1]) + (6, 6), dtype=torch.float64, device=S.device)
    sx, sy, sz = S[..., S_T], S[..., S_T + 1], S[..., S_T + 2]
    L[..., 0, 0] = S[..., S_YY] + S[..., S_ZZ]
    L[..., 1, 1] = S[..., S_XX] + S[..., S_ZZ]
    L[..., 2, 2] = S[..., S_XX] + S[..., S_YY]
    L[..., 0, 1] = L[..., 1, 0] = -S[..., S_XY]
    L[..., 0, 2] = L[..., 2, 0] = -S[..., S_XZ]
    L[..., 1, 2] = L[..., 2, 1] = -S[..., S_YZ]
    L[..., 0, 4] = L[..., 4, 0] = -sz
    L[..., 0, 5] = L[..., 5, 0] = sy
    L[..., 1, 3] = L[..., 3, 1] = sz
    L[..., 1, 5] = L[..., 5, 1] = -sx
    L[..., 2, 3] = L[..., 3, 2] = -sy
    L[..., 2, 4] = L[..., 4, 2] = sx
    c = counts.to(torch.float64)
    L[..., 3, 3] = c
    L[..., 4, 4] = c
    L[..., 5, 5] = c
    return L


def information_matrix(source, target, T, max_distance, source_rows=None, target_rows=None):
    """The 6x6 information matrix of every pose, Open3D's get_information_matrix_from_point_clouds: rule 8 of evaluate_registration over
    the same matches, rotation first.  Arguments as evaluate_registration; returns (..., 6, 6) float64 with the leading shape of its outputs.
    The moment sums are the kernel's (bit-reproducible); the assembly is torch arithmetic on them."""
    on_cpu, _, lead, sums, counts, _, _, _, _ = _evaluate(source, target, T, max_distance, source_rows, target_rows, False, "information_matrix")
    return _shaped(_assemble(sums, counts), lead, on_cpu, (6, 6))


def best_pose(T, counts, rmse):
    """The best hypothesis of every cloud: the largest count, then the smallest rmse, then the lowest h.

    T (N, H, 4, 4) with counts and rmse (N, H) as evaluate_registration returns them -> best (N,) int64, T_best (N, 4, 4); the single-pair
    forms (H, 4, 4) with (H,) give a 0-d best and a (4, 4) pose.  Torch operations on the caller's device (two stable sorts); nothing is
    read back."""
    what = "best_pose"
    for t, name in ((T, "T"), (counts, "counts"), (rmse, "rmse")):
        if not isinstance(t, torch.Tensor):
            _err(what, "%s must be a tensor, got %s" % (name, type(t).__name__))
    if T.dim() not in (3, 4) or tuple(T.shape[-2:]) != (4, 4):
        _err(what, "T must be (N, H, 4, 4) or (H, 4, 4), got shape %s" % (tuple(T.shape),))
    lead = tuple(T.shape[:-2])
    if lead[-1] < 1:
        _err(what, "T holds no hypothesis, shape %s" % (tuple(T.shape),))
    if tuple(counts.shape) != lead or tuple(rmse.shape) != lead:
        _err(what, "counts and rmse must have shape %s, got %s and %s" % (lead, tuple(counts.shape), tuple(rmse.shape)))
    if counts.dtype.is_floating_point or counts.dtype.is_complex or counts.dtype == torch.bool:
        _err(what, "counts must be integers, got %s" % counts.dtype)
    if not rmse.dtype.is_floating_point:
        _err(what, "rmse must be floating point, got %s" % rmse.dtype)
    if not (T.device == counts.device == rmse.device):
        _err(what, "T, counts and rmse must be on one device, got %s, %s and %s" % (T.device, counts.device, rmse.device))
    single = T.dim() == 3
    Tb, cb, rb = (T[None], counts[None], rmse[None]) if single else (T, counts, rmse)
    by_rmse = torch.argsort(rb.detach(), dim=1, stable=True)                                   # ties keep the lower h first
    by_count = torch.argsort(-cb.to(torch.int64).gather(1, by_rmse), dim=1, stable=True)      # ... and so do equal counts
    best = by_rmse.gather(1, by_count[:, :1]).reshape(-1)
    T_best = Tb[torch.arange(Tb.shape[0], device=T.device), best]
    return (best[0], T_best[0]) if single else (best, T_best)
