"""Farthest-point sampling of batches of clouds, with gradients to the sampled rows.

A fixed number of well-spread points per cloud, on the GPU (libdicp_hip.so: dicp_fps_forward / dicp_fps_backward) -- what a voxel grid,
which gives every cloud another row count, does not provide:

    from dicp_amd.fps import sample_farthest_points
    cent, rows = voxel_downsample(scan, 0.1)
    src, idx, src_rows = sample_farthest_points(cent, 1024, rows=rows, return_rows=True)      # (N, 1024, c)
    out = ICP(icp_type="pt2pt").icp(src, target, T0, source_rows=src_rows)

Nothing is read back from the device: the output size is k, so a call on device tensors (an int start, device row counts) can sit inside a
captured region (dicp_amd.graphed); a list, CPU rows / start tensors and start="random" add a host-to-device copy.
"""
import torch

from . import _clouds, _lib
from ._clouds import SLOT, CLOUD
from ._ops import _DT, _p, _workspace

T = 1024                                                    # threads of the resident workgroup (one per cloud)
NR = {torch.float32: 16 * T, torch.float64: 8 * T}          # the largest cloud of the resident form: 16 / 8 rows a thread in registers
STREAM_ROWS = 2048                                          # rows per workgroup of the streamed form
_FORMS = {None: _lib.FPS_AUTO, "resident": _lib.FPS_RESIDENT, "streamed": _lib.FPS_STREAMED}
_RANDOM_HIGH = 2 ** 62


def _scatter(g, idx, shape):
    """the backward's one library call: zeros (N,n,c) with g's rows written at idx"""
    N, n, c, k = shape
    grad = torch.empty((N, n, c), dtype=g.dtype, device=g.device)
    _lib.call("dicp_fps_backward", g.device, _DT[g.dtype], _p(g), _p(idx), N, n, k, c, _p(grad))
    return grad


class _Fps(torch.autograd.Function):
    """(N,n,c) points -> (picked rows (N,k,c), idx (N,k) int64, k_eff (N) int32, distances (N,k)): one library call on the current stream."""

    @staticmethod
    def forward(ctx, pts, rows, start, k, form):
        N, n, c = pts.shape
        dt = _DT[pts.dtype]
        lib = _lib.load()
        dev = pts.device
        out = torch.empty((N, k, c), dtype=pts.dtype, device=dev)
        idx = torch.empty((N, k), dtype=torch.int64, device=dev)
        dist = torch.empty((N, k), dtype=pts.dtype, device=dev)
        keff = torch.empty(N, dtype=torch.int32, device=dev)
        ws_bytes = lib.dicp_fps_workspace_bytes(dt, N, n, k, form)
        ws = _workspace(ws_bytes, dev) if ws_bytes else None
        _lib.call("dicp_fps_forward", dev, dt, _p(pts), c, _p(rows), _p(start), N, n, k, form, _p(out), _p(idx), _p(dist), _p(keff), _p(ws), ws_bytes)
        ctx.save_for_backward(idx)
        ctx.shape = (N, n, c, k)
        ctx.mark_non_differentiable(idx, keff, dist)
        ctx.set_materialize_grads(False)
        return out, idx, keff, dist

    @staticmethod
    def backward(ctx, g_out, _g_idx, _g_keff, _g_dist):
        if g_out is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        idx, = ctx.saved_tensors
        return _scatter(g_out.contiguous(), idx, ctx.shape), None, None, None, None


def _err(msg):
    raise ValueError("sample_farthest_points: " + msg)


def _start(start, N):
    """-> None (row 0), an int > 0, or an (N,) int64 tensor (on the CPU unless it was given on a device)"""
    if isinstance(start, str):
        if start != "random":
            _err("start must be an int >= 0, %d integers or \"random\", got %r" % (N, start))
        return torch.randint(0, _RANDOM_HIGH, (N,), dtype=torch.int64)
    if isinstance(start, torch.Tensor):
        s = start
        if s.dtype.is_floating_point or s.dtype.is_complex or s.dtype == torch.bool or s.dim() != 1 or s.numel() != N:
            _err("start must be %d integers" % N)
        if not s.is_cuda and N and int(s.min()) < 0:
            _err("start must be >= 0")
        return s.to(torch.int64)
    if isinstance(start, bool) or not isinstance(start, int) or start < 0 or start >= 2 ** 63:
        _err("start must be an int >= 0, %d integers or \"random\", got %r" % (N, start))
    return start if start else None


def sample_farthest_points(points, k, rows=None, start=0, return_rows=False, return_distances=False, _form=None):
    """k farthest-point samples of every cloud, on the GPU, with gradients back to the sampled rows.

    points: one cloud (n, c), a padded batch (N, n, c) with optional integer row counts rows (N,), or a list of (n_b, c) clouds; float32 or
        float64, c >= 3.  Columns 0:3 measure distance; all c columns are carried to the output (normals and features travel with the
        point).  CPU tensors are computed on the GPU and returned on the CPU.
    k: an int >= 1.
    start: the row pick 0 starts from -- an int >= 0, an integer (N,) tensor, or "random": ONE draw torch.randint(0, 2**62, (N,)) from
        torch's global (CPU) generator per call; cloud b starts from row draw[b] mod n_b.

    Definition (what the tests pin, index for index):
      - d2(a, b) = (xx + yy) + zz with dx = b.x - a.x, xx = dx * dx (and so on), in the points' dtype, every operation rounded separately
        (no fused multiply-add): the rule of knn_points;
      - the candidates of cloud b are the rows j < rows[b] whose three coordinates are all finite; k_eff = min(k, #candidates);
      - pick 0 is the candidate that minimises (j - start_b) mod n_b with n_b = rows[b]: row start_b mod n_b itself when it is a candidate,
        otherwise the next candidate after it, wrapping round;
      - pick t >= 1: with D_j the minimum of d2(p_j, p_s) over the earlier picks s, the candidate not picked yet with the largest D_j, the
        LOWEST index among equals.  +inf from a float32 overflow is an ordinary value under this rule;
      - output slots at or past k_eff hold idx = -1 and zero rows (every slot of an empty cloud).
    So a cloud's indices are distinct; with k >= #candidates the picks are a permutation of the candidates (duplicate points are picked at
    D = 0 in index order); and the picks' distances never increase from pick 1 on.

    Returns (pts, idx[, k_eff][, distances]): pts (..., k, c) in the input dtype, idx (..., k) int64.  List input: lists of (min(k, n_b), c)
    and (min(k, n_b),).  return_rows adds k_eff, (N,) int32 computed on the device (a 0-d tensor for a single cloud): the source_rows= /
    rows= argument of ICP.icp, estimate_normals and knn_points.  return_distances adds (..., k) in the input dtype: the D of each pick at
    the moment it was picked, the squared coverage radius; +inf for pick 0 and for unused slots.

    Gradients: pts is a gather, so its cotangent goes back to the picked rows of points (all c columns) and every other row gets zero --
    a plain scatter without float atomics (indices are distinct per cloud), bit-reproducible.  idx, k_eff and the distances carry none.

    Two kernels, chosen by size: clouds of up to NR[dtype] rows (16384 float32, 8192 float64) take the resident form -- one workgroup of T
    threads per cloud, the cloud in registers for all k steps; larger clouds the streamed form, one launch per step.  Both give the same
    results.  A call enqueues its work on the current stream and reads nothing back; only rows / start given as CPU tensors are checked
    on the host.  With device tensors, an int start and device (or no) rows the call is kernels only and can be captured in a graph; a list
    of clouds (its row counts), CPU rows / start tensors and start="random" (the draw) each add a host-to-device copy, which cannot.
    """
    if isinstance(k, bool) or not isinstance(k, int) or k < 1 or k > 2 ** 31 - 1:
        _err("k must be an int >= 1, got %r" % (k,))
    if _form not in _FORMS:
        _err("_form must be None, \"resident\" or \"streamed\", got %r" % (_form,))
    form, batch, rows, lens = _clouds.check(points, rows, "sample_farthest_points", empty_ok=True)
    N, n = batch.shape[0], batch.shape[1]
    if _form == "resident" and n > NR[batch.dtype]:
        _err("the resident form holds at most %d rows of %s, got %d" % (NR[batch.dtype], batch.dtype, n))
    start_t = _start(start, N)

    on_cpu, x, rows_d = _clouds.place(batch, rows)
    dev = x.device
    if isinstance(start_t, int):                            # (filled on the device: no host-to-device copy)
        start_d = torch.full((N,), start_t, dtype=torch.int64, device=dev)
    else:
        start_d = start_t.to(device=dev).contiguous() if start_t is not None else None
    pts, idx, keff, dist = _Fps.apply(x, rows_d, start_d, k, _FORMS[_form])
    outs = [(SLOT, pts), (SLOT, idx)] + ([(CLOUD, keff)] if return_rows else []) + ([(SLOT, dist)] if return_distances else [])
    return _clouds.restore(form, on_cpu, n, lens, outs, k=k)
