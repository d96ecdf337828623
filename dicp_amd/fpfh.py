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

Not built: gradients (the bins are piecewise constant: the outputs never require grad), k > 32, other descriptors (SHOT), and a ball query
fused into the first pass.
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


def compute_fpfh(points, normals, radius, k=32, rows=None):
    """fpfh_features over the neighbours within `radius`: idx = ball_query(points, points, radius, k, x_rows=rows, y_rows=rows), the
    nearest k of them, then fpfh_features(points, normals, idx, rows=rows, radius=radius).

    points, normals, rows: as fpfh_features.  radius: a finite Python float > 0.  k: an int in [1, 32]; a point finds itself first, so
    k - 1 slots are left for its neighbours.  Returns the descriptors in the form of the points."""
    what = "compute_fpfh"
    if radius is None:
        raise ValueError("%s: radius must be a finite float > 0, got None" % what)
    radius = _check_radius(radius, what)
    _clouds._check_k(k, what, K_MIN, K_MAX)
    form, batch, _, lens = _clouds.check(points, rows, what)
    _clouds.check_table(normals, what, "normals", (form, batch, lens), 3)
    with torch.no_grad():
        idx = ball_query(points, points, radius, k=k, x_rows=rows, y_rows=rows)[1]
    return fpfh_features(points, normals, idx, rows=rows, radius=radius)
