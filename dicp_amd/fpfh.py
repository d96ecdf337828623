"""FPFH descriptors (Fast Point Feature Histograms, Rusu, Blodow and Beetz 2009; 33 channels) from points, normals and neighbours.

The descriptor stage of a classical global registration, on the GPU (libdicp_hip.so: dicp_fpfh_spfh / dicp_fpfh_combine; the rules:
csrc/dicp_fpfh.h).  Its inputs are what the other operators produce -- points, the unit normals of estimate_normals, and the (N, m, k) index
tensor of a search of every cloud against itself, with -1 in empty slots -- and its output is what match_features takes:

    from dicp_amd.fpfh import compute_fpfh
    nx = estimate_normals(x, k=16, viewpoint=eye_x)            # the normals must be ORIENTED: see below
    ny = estimate_normals(y, k=16, viewpoint=eye_y)
    fx, fy = compute_fpfh(x, nx, 0.8), compute_fpfh(y, ny, 0.8)
    idx, _ = match_features(fx, fy, mutual=True)
    T0, inliers = ransac_correspondences(x, y, idx, 0.1)       # -> ICP(...).icp(x, y, T_init=T0)

FPFH is invariant to a rigid motion of points AND normals together, not to flipping a normal: a normal and its negative fall into
different bins.  Two scans of one scene therefore need consistently oriented normals -- each towards its own sensor position
(estimate_normals(viewpoint=), the moved scan with the moved viewpoint).

The k-slot form (fpfh_features / compute_fpfh by default) sees at most the k <= 32 slots of the index.  The whole-ball form
(fpfh_features_ball / compute_fpfh(whole_ball=True); libdicp_hip.so: dicp_fpfh_ball_pack / _spfh / _combine, the near list:
csrc/dicp_fpfh_ball.h) walks EVERY row of the ball on the cloud's cell grid, takes no index, and can describe chosen rows only (at=): the
keypoints of compute_iss_keypoints(return_index=True, whole_ball=True).

Not built: gradients (the bins are piecewise constant: the outputs never require grad), other descriptors (SHOT), a ball query fused into
the first pass of the k-slot form, at= for the k-slot form.
"""
import math

import torch

from . import _clouds, _lib
from ._clouds import ROW
from ._ops import _DT, _p, _workspace
from .ball import ball_query

K_MIN, K_MAX = 1, 32                # FPFH_K_MIN, FPFH_K_MAX (csrc/dicp_fpfh.h): the slots of idx
CHANNELS, BINS = 33, 11             # theta in [0, 11), alpha in [11, 22), phi in [22, 33)
ROW_BYTES = 48                      # FPFH_ROW_BYTES: a row of the internal table between the two passes


def _check_radius(radius, what):
    """None or a finite Python number > 0 -> the float the library takes (0.0: no radius)"""
    if radius is None:
        return 0.0
    ok = not isinstance(radius, bool) and isinstance(radius, (int, float))
    if ok:
        try:
            radius = float(radius)
        except OverflowError:
            ok = False
    if not ok or not (math.isfinite(radius) and radius > 0.0):
        raise ValueError("%s: radius must be None or a finite float > 0, got %r" % (what, radius))
    return radius


def _fpfh(x, nrm, idx, rows_d, radius, want_spfh):
    """placed arguments -> (out (N,m,33) in x's dtype, spfh (N,m,33) uint8 or None): two launches on the current stream"""
    N, m, c = x.shape
    k = idx.shape[2]
    dev = x.device
    ws_bytes = _lib.load().dicp_fpfh_workspace_bytes(N, m)
    if ws_bytes == 0:
        raise ValueError("fpfh_features: N * m must stay below 2^31, got N = %d, m = %d" % (N, m))
    ws = _workspace(ws_bytes, dev)
    out = torch.empty((N, m, CHANNELS), dtype=x.dtype, device=dev)
    spfh = torch.empty((N, m, CHANNELS), dtype=torch.uint8, device=dev) if want_spfh else None
    i64 = 1 if idx.dtype == torch.int64 else 0
    _lib.call("dicp_fpfh_spfh", dev, _DT[x.dtype], _p(x), c, _p(nrm), _p(idx), i64, _p(rows_d), N, m, k, radius, _p(ws), ws_bytes, _p(spfh))
    _lib.call("dicp_fpfh_combine", dev, _DT[x.dtype], _p(x), c, _p(idx), i64, _p(rows_d), N, m, k, radius, _p(ws), ws_bytes, _p(out))
    return out, spfh


def fpfh_features(points, normals, idx, rows=None, radius=None, return_spfh=False):
    """The 33-channel FPFH descriptor of every point, on the GPU.

    points: (m, c), (N, m, c) or a list of (m_b, c) with c >= 3; float32 or float64; columns 0:3 are the coordinates, the others are not
        read.  CPU tensors are computed on the GPU and returned on the CPU.
    normals: (m, 3) / (N, m, 3) / a list of (m_b, 3) in the same form, dtype and device.  They are used as they are (not normalised).
    idx: the neighbours of every point IN ITS OWN CLOUD -- the idx of ball_query(p, p, ...) or knn_points(p, p, ...): (m, k), (N, m, k) or a
        list of (m_b, k), int64 or int32, 1 <= k <= 32, on the points' device.  A slot is empty when its index is negative or at or past
        the cloud's row count; the row itself is skipped wherever it stands.  The kernels never read out of range whatever idx holds.
    rows: optional (N,) row counts of a padded batch.
    radius: None, or a finite Python float > 0: slots whose d2, RECOMPUTED here in double, exceeds radius * radius are dropped -- a
        knn_points index used as a "hybrid" search.
    Anything else is a ValueError before any device work.

    Definition (csrc/dicp_fpfh.h states every operation; tests/fpfh_ref.py is its numpy restatement).  All arithmetic is in double on the
    exactly converted inputs, with + - * / sqrt only.  A row is OK when its coordinates and normal are finite and the normal is not zero.
    Slot (i, s) naming row j is NEAR when both rows are OK, j != i, r2 = |p_j - p_i|^2 > 0 and r2 <= radius^2; a near slot is a PAIR when its
    Darboux frame exists.  For a pair (Open3D's ComputePairFeatures): d = p_j - p_i, a1 = n_i.d / r, a2 = n_j.d / r; the point with the
    smaller |angle| becomes the source (a tie keeps i); v = d x n1 normalised, w = n1 x v; theta = the angle of (n1.n2, w.n2),
    alpha = v.n2, phi = n1.d / r.  Each feature has 11 bins (theta over (-pi, pi], decided by half-plane tests, no atan2).
      SPFH: s_i[ch] = 100 cnt[i, ch] / c_i over the c_i pairs of row i (0 without one).
      FPFH: acc[ch] = sum over the near slots, in slot order, of s_j[ch] / r2; out[ch] = 100 acc[ch] / (the sum of acc over the feature's
      11 channels) + s_i[ch], rounded once to the points' dtype; 0 where that sum is 0.  Every feature of a row with neighbours sums to 200.
    Rows that are not OK, and rows at or past rows[b], get 33 zeros.

    Returns out (m, 33) / (N, m, 33) / a list of (m_b, 33) in the points' dtype; with return_spfh=True (out, spfh), spfh the integer bin
    counts cnt of the first pass as contiguous uint8 in the same form.

    No gradients: the bins are piecewise constant in the inputs, so the outputs never require grad.  Nothing is read back from the device
    and both launches are on the current stream: a call on device tensors with device (or no) rows can sit in a captured graph.  No float
    atomics: the result is bit-reproducible and does not depend on which search produced idx beyond the indices themselves.
    """
    what = "fpfh_features"
    if not isinstance(return_spfh, bool):
        raise ValueError("%s: return_spfh must be True or False, got %r" % (what, return_spfh))
    radius = _check_radius(radius, what)
    form, batch, rows, lens = _clouds.check(points, rows, what)
    nb = _clouds.check_table(normals, what, "normals", (form, batch, lens), 3)
    ib, ilens = _clouds.check_slots(idx, what, "idx", (form, batch), True, K_MIN, K_MAX)
    if ib.shape[1] != batch.shape[1] or (lens is not None and list(ilens) != list(lens)):
        raise ValueError("%s: idx must be a search of the cloud against itself, one row of slots per point: got %s rows for %s points"
                         % (what, ilens if lens is not None else ib.shape[1], lens if lens is not None else batch.shape[1]))
    on_cpu, x, rows_d = _clouds.place(batch, rows)
    out, spfh = _fpfh(x.detach(), nb.detach().to(x.device).contiguous(), ib.to(x.device).contiguous(), rows_d, radius, return_spfh)
    outs = _clouds.restore(form, on_cpu, batch.shape[1], lens, [(ROW, out)] + ([(ROW, spfh)] if return_spfh else []))
    return outs if return_spfh else outs[0]


# ------------------------------------------------------------------ the whole-ball form
def _check_at(at, what, form, batch):
    """The rows to describe, in the form of the points: (q,), (N, q) or a list of (q_b,), int32 or int64, on the points' device
    -> (batch (N, q), the q_b of a list or None); a list is padded with -1, a dead entry.  ValueError for anything invalid."""
    is_list = isinstance(at, (list, tuple))
    items = list(at) if is_list else [at]
    if is_list and not items:
        raise ValueError("%s: at is an empty list" % what)
    for i, c in enumerate(items):
        nm = "at[%d]" % i if is_list else "at"
        if not isinstance(c, torch.Tensor):
            raise ValueError("%s: %s must be a tensor, got %s" % (what, nm, type(c).__name__))
        if c.dtype not in (torch.int32, torch.int64):
            raise ValueError("%s: %s must be int32 or int64, got %s" % (what, nm, c.dtype))
        if c.device != batch.device:
            raise ValueError("%s: %s and the points must be on one device, got %s and %s" % (what, nm, c.device, batch.device))
        if is_list and c.dim() != 1:
            raise ValueError("%s: %s must be (q_b,), got shape %s" % (what, nm, tuple(c.shape)))
    if not is_list and at.dim() not in (1, 2):
        raise ValueError("%s: at must be (q,), (N, q) or a list of (q_b,), got shape %s" % (what, tuple(at.shape)))
    mine = "list" if is_list else ("single" if at.dim() == 1 else "batch")
    if mine != form:
        raise ValueError("%s: at must have the form of the points (single clouds, padded batches or lists), got %s and %s" % (what, mine, form))
    if len({c.dtype for c in items}) != 1:
        raise ValueError("%s: the clouds of at need one dtype" % what)
    if is_list:
        ab, lens = torch.nn.utils.rnn.pad_sequence(items, batch_first=True, padding_value=-1), [c.shape[0] for c in items]
    else:
        ab, lens = (at.unsqueeze(0) if at.dim() == 1 else at), None
    if ab.shape[0] != batch.shape[0]:
        raise ValueError("%s: at and the points must hold the same number of clouds, got %d and %d" % (what, ab.shape[0], batch.shape[0]))
    if ab.shape[1] < 1 or ab.shape[0] * ab.shape[1] >= 2 ** 31:
        raise ValueError("%s: at needs at least one entry and N * q below 2^31, got shape %s" % (what, tuple(ab.shape)))
    return ab, lens


def _fpfh_ball(x, nrm, rows_d, radius, at, want_spfh, what):
    """placed arguments -> (out (N,m,33) or (N,q,33) in x's dtype, spfh (N,m,33) int32 or None): the grid build and three launches on the
    current stream"""
    from .iss import _ball_grid
    N, m, _ = x.shape
    dev, dt = x.device, _DT[x.dtype]
    ws_bytes = _lib.load().dicp_fpfh_ball_workspace_bytes(dt, N, m)
    if ws_bytes == 0:
        raise ValueError("%s: N * m must stay below 2^31, got N = %d, m = %d" % (what, N, m))
    grid = _ball_grid(x, rows_d, radius)
    ws = _workspace(ws_bytes, dev)
    q = 0 if at is None else at.shape[1]
    out = torch.empty((N, m if at is None else q, CHANNELS), dtype=x.dtype, device=dev)
    spfh = torch.empty((N, m, CHANNELS), dtype=torch.int32, device=dev) if want_spfh else None
    g = (_p(grid.plans), _p(grid.keys), _p(grid.perm), _p(grid.rows4))
    _lib.call("dicp_fpfh_ball_pack", dev, dt, g[0], g[2], g[3], _p(nrm), N, m, _p(ws), ws_bytes)
    _lib.call("dicp_fpfh_ball_spfh", dev, dt, *g, N, m, radius, _p(ws), ws_bytes, _p(spfh), None)
    _lib.call("dicp_fpfh_ball_combine", dev, dt, *g, _p(at), 1 if at is not None and at.dtype == torch.int64 else 0, q, N, m, radius, _p(ws), ws_bytes,
              _p(out), None)
    return out, spfh


def fpfh_features_ball(points, normals, radius, rows=None, at=None, return_spfh=False):
    """The 33-channel FPFH descriptor over EVERY row of each point's ball, Open3D's neighbourhood: fpfh_features without an index and
    without its limit of 32 slots -- for every row, or only for the rows `at` names.

    points, normals, rows: as fpfh_features.  radius: required, a finite Python float > 0 whose square is finite.
    at: None for a descriptor of every row, or the rows to describe as indices into the SAME cloud: (q,), (N, q) or a list of (q_b,) in
        the form of the points, int64 or int32, on the points' device -- the `index` of select_rows / compute_iss_keypoints(return_index=
        True) goes in unchanged.  An entry is live when 0 <= at[e] < rows[b]; every other entry gets 33 zeros, and nothing is read out of
        range whatever at holds.  Duplicates are allowed.
    Anything else is a ValueError before any device work.

    Definition (csrc/dicp_fpfh_ball.h; tests/fpfh_ball_ref.py is its numpy restatement).  Everything of fpfh_features stands; only the
    neighbour list changes: the near list of an OK row i is ALL other OK rows j < rows[b] of the cloud with 0 < (dx dx + dy dy) + dz dz <=
    radius radius in double on the exactly converted inputs (exact duplicates are not near), in ascending (cell key, row index) order of
    the cloud's cell grid -- the grid ball_query builds (csrc/dicp_ball.h), at the radius rounded UP to the points' dtype, as
    iss_saliency_ball.  The weighted sum runs over the near list in that order.  The bin counts are 32-bit.

    Returns out (m, 33) / (N, m, 33) / a list of (m_b, 33) in the points' dtype -- with at: (q, 33) / (N, q, 33) / a list of (q_b, 33),
    entry e the descriptor of row at[e]; with return_spfh=True (out, spfh), spfh the bin counts of the first pass as contiguous int32
    (m, 33) / (N, m, 33) / a list, for EVERY row whatever at is.

    One grid build and three launches on the current stream; no index or distance tensor exists at any point.  The first pass always
    covers every row (a row's descriptor needs the counts of all rows of its ball); the second walks only the rows asked for.  No
    gradients: the outputs never require grad.  Nothing is read back (a call on device tensors with device or no rows can sit in a
    captured graph); no float atomics: bit-reproducible.
    """
    from .iss import _check_ball_radius
    what = "fpfh_features_ball"
    if not isinstance(return_spfh, bool):
        raise ValueError("%s: return_spfh must be True or False, got %r" % (what, return_spfh))
    r = _check_ball_radius(radius, what, "radius")
    form, batch, rows, lens = _clouds.check(points, rows, what)
    nb = _clouds.check_table(normals, what, "normals", (form, batch, lens), 3)
    ab, qlens = (None, None) if at is None else _check_at(at, what, form, batch)
    on_cpu, x, rows_d = _clouds.place(batch, rows)
    at_d = None if ab is None else ab.to(x.device).contiguous()
    out, spfh = _fpfh_ball(x.detach(), nb.detach().to(x.device).contiguous(), rows_d, r, at_d, return_spfh, what)
    if ab is None:
        outs = _clouds.restore(form, on_cpu, batch.shape[1], lens, [(ROW, out)] + ([(ROW, spfh)] if return_spfh else []))
        return outs if return_spfh else outs[0]
    if on_cpu:
        out = out.cpu()
    out = [out[b, :n] for b, n in enumerate(qlens)] if form == "list" else (out[0] if form == "single" else out)
    return (out, _clouds.restore(form, on_cpu, batch.shape[1], lens, [(ROW, spfh)])[0]) if return_spfh else out


def compute_fpfh(points, normals, radius, k=32, rows=None, whole_ball=False, at=None):
    """fpfh_features over the neighbours within `radius`: idx = ball_query(points, points, radius, k, x_rows=rows, y_rows=rows), the
    nearest k of them, then fpfh_features(points, normals, idx, rows=rows, radius=radius).  With whole_ball=True:
    fpfh_features_ball(points, normals, radius, rows=rows, at=at) -- every row of the ball, no index; k is checked but not used.

    points, normals, rows: as fpfh_features.  radius: a finite Python float > 0.  k: an int in [1, 32]; a point finds itself first, so
    k - 1 slots are left for its neighbours.  whole_ball: True or False.  at: with whole_ball=True only (a ValueError otherwise), the
    rows to describe, as fpfh_features_ball takes them.  Returns the descriptors in the form of the points (of at, where given)."""
    what = "compute_fpfh"
    if not isinstance(whole_ball, bool):
        raise ValueError("%s: whole_ball must be True or False, got %r" % (what, whole_ball))
    if radius is None:
        raise ValueError("%s: radius must be a finite float > 0, got None" % what)
    radius = _check_radius(radius, what)
    _clouds._check_k(k, what, K_MIN, K_MAX)
    form, batch, _, lens = _clouds.check(points, rows, what)
    _clouds.check_table(normals, what, "normals", (form, batch, lens), 3)
    if at is not None and not whole_ball:
        raise ValueError("%s: at needs whole_ball=True (the k-slot form describes every row)" % what)
    if whole_ball:
        from .iss import _check_ball_radius
        _check_ball_radius(radius, what, "radius")
        if at is not None:
            _check_at(at, what, form, batch)
        return fpfh_features_ball(points, normals, radius, rows=rows, at=at)
    with torch.no_grad():
        idx = ball_query(points, points, radius, k=k, x_rows=rows, y_rows=rows)[1]
    return fpfh_features(points, normals, idx, rows=rows, radius=radius)
