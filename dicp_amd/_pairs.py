"""What the operators on explicit correspondences share (register.py: poses; compat.py: pruning): the checks of their arguments, the pose
layouts, and the packed-pair record -- the one place that knows how a cloud's live pairs are packed and how a packed result goes back to
the original rows.  _number is also the number check of match.py.
"""
import torch

from . import _clouds
from .filter import _Select


_INF = float("inf")


def _number(value, what, tail, lo=None, hi=None, lo_open=False, hi_open=False, integer=False, none_ok=False, fmt=None):
    """ValueError "<what>: <tail>, got <value>" unless value is a Python int (integer=True) or an int or float -- a bool is neither -- within
    lo .. hi, an end being excluded where it is open; a float is compared as float(value), so a NaN fails every bound.  none_ok: None passes.
    fmt: what tail is to be formatted with (only a refused value pays for its message)."""
    if value is None and none_ok:
        return
    ok = not isinstance(value, bool) and isinstance(value, int if integer else (int, float))
    if ok:
        v = value if integer else float(value)
        ok = (lo is None or (lo < v if lo_open else lo <= v)) and (hi is None or (v < hi if hi_open else v <= hi))
    if not ok:
        raise ValueError("%s: %s, got %r" % (what, tail if fmt is None else tail % fmt, value))


def _flag(value, what, name):
    if not isinstance(value, bool):
        raise ValueError("%s: %s must be True or False, got %r" % (what, name, value))


def _int_in(value, what, name, lo, hi):
    _number(value, what, "%s must be an int in [%d, %d]", lo, hi, integer=True, fmt=(name, lo, hi))


def _threshold(value, what, name="threshold", none_ok=False):
    """the check of a distance: a finite number > 0"""
    _number(value, what, "%s must be %sa finite number > 0", 0.0, _INF, True, True, none_ok=none_ok, fmt=(name, "None or " if none_ok else ""))


_NO_T = object()


def _pair_arguments(x, y, idx, weight, x_rows, what, T=_NO_T):
    """The checks of align_correspondences (and of a transform T, where one is given; ValueError before any device work), then its
    arguments on the device:
    -> (form, on_cpu, x (N,n,3), y (N,m,3), idx (N,n) as given, weight (N,n) or None, rows (N,) int32 or None)."""
    (form, bx, rx, _), (_, by, _, _) = _clouds.check_pair(x, y, x_rows, None, what)
    if form == "list":
        raise ValueError("%s: x and y must be single clouds or padded batches" % what)
    if bx.shape[1] < 1 or by.shape[1] < 1:
        raise ValueError("%s: x and y need at least one row" % what)
    N, n, m = bx.shape[0], bx.shape[1], by.shape[1]
    if not isinstance(idx, torch.Tensor) or idx.dtype not in (torch.int32, torch.int64):
        raise ValueError("%s: idx must be an int32 or int64 tensor, got %s" % (what, getattr(idx, "dtype", type(idx).__name__)))
    if tuple(idx.shape) != ((n,) if form == "single" else (N, n)) or idx.device != bx.device:
        raise ValueError("%s: idx must hold one entry per row of x on x's device, shape %s, got %s on %s"
                         % (what, (n,) if form == "single" else (N, n), tuple(idx.shape), idx.device))
    if not idx.is_cuda and idx.numel() and int(idx.max()) >= m:
        raise ValueError("%s: idx must be below y's %d rows" % (what, m))
    if weight is not None:
        if not isinstance(weight, torch.Tensor) or weight.dtype != bx.dtype or tuple(weight.shape) != tuple(idx.shape) or weight.device != bx.device:
            raise ValueError("%s: weight must be a tensor of x's dtype and device with idx's shape" % what)
    if T is not _NO_T:
        shape = (4, 4) if form == "single" else (N, 4, 4)
        if not isinstance(T, torch.Tensor) or T.dtype != bx.dtype or tuple(T.shape) != shape or T.device != bx.device:
            raise ValueError("%s: T must be a %s tensor of x's dtype on x's device" % (what, shape))
    on_cpu, xd, rows = _clouds.place(bx, rx, xyz=False)
    _, yd, _ = _clouds.place(by, None, xyz=False)
    dev = xd.device
    xd, yd = xd[..., :3].contiguous(), yd[..., :3].contiguous()
    idx_d = idx.to(dev).reshape(N, n)
    return form, on_cpu, xd, yd, idx_d, None if weight is None else weight.to(dev).reshape(N, n), rows


def _finish(form, on_cpu, outs, per_row):
    """An operator's (N, ...) results as the caller gets them -> a tuple: on the CPU where the arguments were, and for a single pair of
    clouds the first per_row of them without their leading axis (the others have no per-row axis and stay (N, ...))."""
    if on_cpu:
        outs = [t.cpu() for t in outs]
    if form == "single":
        outs = [t[0] for t in outs[:per_row]] + list(outs[per_row:])
    return tuple(outs)


def _pose12(T):
    """(N, 4, 4) -> (N, 12): C row-major, then r"""
    return torch.cat((T[:, :3, :3].reshape(-1, 9), T[:, :3, 3]), dim=1).contiguous()


def _T44(pose):
    """(N, 12) -> (N, 4, 4)"""
    N = pose.shape[0]
    T = torch.zeros((N, 4, 4), dtype=pose.dtype, device=pose.device)
    T[:, :3, :3] = pose[:, :9].reshape(N, 3, 3)
    T[:, :3, 3] = pose[:, 9:]
    T[:, 3, 3] = 1.0
    return T


def _idx32(idx_d, m):
    """idx as the kernels read it: int32, anything at or past m clamped to m (the kernels clamp into [0, m - 1])"""
    return idx_d.clamp(min=-1, max=m).to(torch.int32).contiguous()


def _mask_idx(mask, idx_d):
    """idx where the mask holds, -1 elsewhere"""
    return torch.where(mask, idx_d, torch.full_like(idx_d, -1))


class _Pairs:
    """The live pairs of every cloud, packed first in ascending row order (_live_pairs): idx32 (N, n), live (N, n) bool, pairs (N, n, 6):
    (x[0:3], y[0:3]), u (N, n): the packed user weights, or None, P (N,) int32, index (N, n) int64: the row of every packed pair, or None."""
    __slots__ = ("idx32", "live", "pairs", "u", "P", "index", "_pos")

    def __init__(self, idx32, live, pairs, u, P, index):
        self.idx32, self.live, self.pairs, self.u, self.P, self.index, self._pos = idx32, live, pairs, u, P, index, None

    def _rows(self, t):
        """packed (N, n) -> every row the entry at its packed position (a row that is not live: some live row's)"""
        if self._pos is None:
            self._pos = (torch.cumsum(self.live, dim=1) - 1).clamp(min=0)      # the packed position of every live row
        return torch.gather(t, 1, self._pos)

    def unpack(self, t):
        """packed (N, n) -> the original row order, 0 on rows that are not live"""
        return torch.where(self.live, self._rows(t), torch.zeros((), dtype=t.dtype, device=t.device))

    def keep(self, rank, keep, idx_d):
        """rule 5 of prune_correspondences on packed ranks (N, n) int32 -> (kept (N, n) bool, idx_kept)"""
        kept = self.live & (self._rows(rank) < min(int(keep), 0x7fffffff))
        return kept, _mask_idx(kept, idx_d)


def _live_pairs(x0, y0, idx_d, rows, weight=None):
    """Rule 1 of ransac_correspondences on detached (N, n, 3) / (N, m, 3) points -> _Pairs.  With a weight (N, n), rule 1 of
    gnc_correspondences: its own condition joins, it rides along as a seventh column into u, and no index is asked for."""
    N, n, _ = x0.shape
    m, dev = y0.shape[1], x0.device
    idx32 = _idx32(idx_d, m)
    yg = torch.gather(y0, 1, idx32.clamp(min=0, max=m - 1).long()[..., None].expand(N, n, 3))
    live = (idx32 >= 0) & torch.isfinite(x0).all(dim=-1) & torch.isfinite(yg).all(dim=-1)
    if weight is not None:
        live = live & torch.isfinite(weight) & (weight > 0)
    if rows is not None:
        live &= torch.arange(n, device=dev)[None, :] < rows[:, None]
    cols = (x0, yg) if weight is None else (x0, yg, weight[..., None])
    packed, P, index = _Select.apply(torch.cat(cols, dim=-1).contiguous(), live.contiguous(), None, weight is None)
    if weight is None:
        return _Pairs(idx32, live, packed, None, P, index)
    return _Pairs(idx32, live, packed[..., :6].contiguous(), packed[..., 6].contiguous(), P, index)
