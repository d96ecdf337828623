"""Differentiable voxel-grid downsampling of batches of clouds.

A raw scan is reduced to one centroid per occupied voxel, on the GPU (libdicp_hip.so: dicp_voxel_count / dicp_voxel_reduce /
dicp_voxel_backward), with gradients back to the points.  The result is a zero-padded batch with per-cloud row counts, the form
`estimate_normals(..., rows=)` and `ICP.icp(..., source_rows=, target_rows=)` take:

    from dicp_amd.voxel import voxel_downsample
    cent, rows = voxel_downsample(points, 0.1)
    nrm = estimate_normals(cent, k=16, rows=rows)
    target = torch.cat((cent, nrm), dim=-1)       # -> ICP(icp_type='pt2pl').icp(..., target_rows=rows)
"""
import numbers

import torch

from . import _clouds, _lib
from ._clouds import ROW, CLOUD, VOXEL
from ._ops import _DT, _p, _workspace

_ERR = {1: "a voxel coordinate |floor((p - origin) / voxel_size)| reaches 2^62",
        2: "its voxel coordinates span more than 64 bits (w_x + w_y + w_z > 64)"}


class _Voxel(torch.autograd.Function):
    """(N,m,c) points -> (centroids (N,M,c), counts (N,M) int32, inverse (N,m) int64, rows_out (N) int32 on the device, on the host): one count
    call, ONE device-to-host read of the N counts and the error word, one reduce call; the backward is one library call."""

    @staticmethod
    def forward(ctx, pts, rows, size, origin, min_points):
        N, m, c = pts.shape
        dt = _DT[pts.dtype]
        lib = _lib.load()
        ws_bytes = lib.dicp_voxel_workspace_bytes(dt, N, m, c)
        ws = _workspace(ws_bytes, pts.device)
        info = torch.empty(N + 1, dtype=torch.int32, device=pts.device)
        _lib.call("dicp_voxel_count", pts.device, dt, _p(pts), c, _p(rows), N, m, size[0], size[1], size[2], _p(origin),
                  int(origin is not None and origin.dim() == 2), min_points, _p(info), _p(ws), ws_bytes)
        host = info.cpu()                                       # the one device -> host read of the call
        err = int(host[N])
        if err:
            raise ValueError("voxel_downsample: cloud %d: %s" % ((err >> 2) - 1, _ERR.get(err & 3, "error %d" % err)))
        M = int(host[:N].max())
        cent = torch.empty((N, M, c), dtype=pts.dtype, device=pts.device)
        counts = torch.empty((N, M), dtype=torch.int32, device=pts.device)
        inverse = torch.empty((N, m), dtype=torch.int64, device=pts.device)
        _lib.call("dicp_voxel_reduce", pts.device, dt, _p(pts), c, N, m, M, _p(ws), ws_bytes, _p(cent) if M else None, _p(counts) if M else None,
                  _p(inverse))
        ctx.save_for_backward(inverse, counts)
        ctx.shape = (N, m, c, M)
        rows_dev, rows_host = info[:N], host[:N]
        ctx.mark_non_differentiable(counts, inverse, rows_dev, rows_host)
        ctx.set_materialize_grads(False)
        return cent, counts, inverse, rows_dev, rows_host

    @staticmethod
    def backward(ctx, g_cent, _g_counts, _g_inverse, _g_rows, _g_host):
        if g_cent is None:
            return None, None, None, None, None
        inverse, counts = ctx.saved_tensors
        N, m, c, M = ctx.shape
        g = g_cent.contiguous()
        grad = torch.empty((N, m, c), dtype=g.dtype, device=g.device)
        _lib.call("dicp_voxel_backward", g.device, _DT[g.dtype], _p(g) if M else None, _p(inverse), _p(counts) if M else None, N, m, M, c, _p(grad))
        return grad, None, None, None, None


def _real_values(x, what):
    """a number, a sequence of numbers or a real tensor -> (its shape, float64 tensor of its values)"""
    bad = ValueError("voxel_downsample: %s must be real numbers, got %r" % (what, x))
    if isinstance(x, bool):
        raise bad
    try:                                                    # (Python numbers straight to float64: as_tensor would round them to float32 first)
        t = x.detach() if isinstance(x, torch.Tensor) else torch.tensor(x, dtype=torch.float64)
    except (TypeError, ValueError, RuntimeError):
        raise bad from None
    if t.dtype == torch.bool or t.dtype.is_complex:
        raise bad
    return tuple(t.shape), t.to(device="cpu", dtype=torch.float64)


def _voxel_size(voxel_size, dtype):
    """-> [sx, sy, sz] as the points' dtype rounds them, each positive and finite"""
    shape, t = _real_values(voxel_size, "voxel_size")
    if shape not in ((), (1,), (3,)):
        raise ValueError("voxel_downsample: voxel_size must be a scalar or (3,), got shape %s" % (shape,))
    t = t.reshape(-1).expand(3)
    rounded = t.to(dtype).to(torch.float64)
    if not (bool(torch.isfinite(t).all()) and bool((t > 0).all()) and bool(torch.isfinite(rounded).all()) and bool((rounded > 0).all())):
        raise ValueError("voxel_downsample: voxel_size must be positive and finite in %s, got %r" % (dtype, voxel_size))
    return [float(v) for v in rounded]


def voxel_downsample(points, voxel_size, rows=None, origin=None, min_points=1, return_counts=False, return_inverse=False):
    """One centroid per occupied voxel of every cloud, on the GPU, with gradients back to the points.

    points: (m, c), (N, m, c) with c >= 3, or a list of (m_b, c); float32 or float64.  CPU tensors are computed on the GPU and returned on
        the CPU.  rows: optional (N,) row counts of a padded batch (rows past them are padding).
    voxel_size: a positive finite scalar or (3,) per-axis sizes.  origin: None (the origin), (3,) or (N, 3).  min_points: an int >= 1.

    Definition (what the tests pin):
      - row r of cloud b takes part when r < rows[b] and its x, y, z are finite; any other row is ignored, whatever it holds (inverse -1);
      - its voxel is v_d = floor((p_d - o_d) / s_d), computed in the points' dtype with o and s first converted to it: one rounded
        subtraction, one IEEE division (numpy computes the same values on arrays of that dtype);
      - a cloud's voxels are its distinct (vx, vy, vz) holding at least min_points rows, in ascending lexicographic order (the order of
        np.unique(coords, axis=0)); the rows of a dropped voxel get inverse -1;
      - a centroid is the mean of ALL c columns of its rows (extra columns such as intensity or weights are averaged too): the sum in
        float64, divided by the count, rounded once to the dtype.  Normals among the columns are averaged but not re-normalised:
        estimate normals after downsampling (dicp_amd.normals.estimate_normals(cent, rows=rows_out));
      - gradient: grad_points[b, i] = grad_centroids[b, inverse[b, i]] / counts[b, inverse[b, i]] (one IEEE division per element by the
        count in the dtype), 0 where the inverse is -1.  voxel_size and origin get none (membership is piecewise constant);
      - forward and backward use no float atomics and are bit-reproducible from run to run (estimate_normals' backward is not).
    Range limit: with w_d = bit_length(max v_d - min v_d) over a cloud's rows, w_x + w_y + w_z > 64 or any |v_d| >= 2^62 raises ValueError
    naming the cloud (at 1 cm voxels only clouds wider than ~20 km on every axis).
    Host synchronisation: a call reads the N voxel counts and an error word back from the device ONCE, to size its outputs; the backward
    reads nothing.  The downsample therefore cannot be captured in a graph.

    Returns (centroids, rows_out[, counts][, inverse]).  Batch input: centroids (N, M, c), M = max(rows_out), zero at and past rows_out[b];
    rows_out (N,) int32; counts (N, M) int32, 0 on pad rows; inverse (N, m) int64 (the row's voxel or -1).  Single-cloud input: every output
    is the batch's cloud 0 -- centroids (M, c), rows_out a 0-d tensor, counts (M,), inverse (m,).  List input: lists of the per-cloud ones.
    """
    if isinstance(min_points, bool) or not isinstance(min_points, numbers.Integral) or min_points < 1 or min_points > 2 ** 31 - 1:
        raise ValueError("voxel_downsample: min_points must be an int >= 1, got %r" % (min_points,))
    form, batch, rows, lens = _clouds.check(points, rows, "voxel_downsample", flat_rows=True)
    N, m = batch.shape[0], batch.shape[1]
    size = _voxel_size(voxel_size, batch.dtype)
    o = None
    if origin is not None:
        shape, t = _real_values(origin, "origin")
        if shape not in ((3,), (N, 3)):
            raise ValueError("voxel_downsample: origin must be (3,) or (%d, 3), got shape %s" % (N, shape))
        o = t.to(batch.dtype)
        if not (bool(torch.isfinite(t).all()) and bool(torch.isfinite(o).all())):
            raise ValueError("voxel_downsample: origin must be finite in %s" % batch.dtype)

    on_cpu, x, rows_d = _clouds.place(batch, rows)
    o_d = o.to(x.device).contiguous() if o is not None else None
    cent, counts, inverse, rows_out, rows_host = _Voxel.apply(x, rows_d, size, o_d, int(min_points))
    outs = [(VOXEL, cent), (CLOUD, rows_out)] + ([(VOXEL, counts)] if return_counts else []) + ([(ROW, inverse)] if return_inverse else [])
    return _clouds.restore(form, on_cpu, m, lens, outs, voxels=rows_host)
