"""The cloud arguments of the point-cloud operators (normals, voxel, knn, fps, ball, group, match, fpfh, iss): one cloud, a padded batch with row counts, or a list.

check / check_pair / check_slots / check_table validate on the host (no device is touched), place moves a checked batch to the compute device, restore
cuts the library's (N, ...) results back to the caller's form and device.  What differs between the operators is an argument at their call
site.
"""
import torch

from ._ops import _DT, compute_device

ROW, SLOT, CLOUD, VOXEL = "row", "slot", "cloud", "voxel"      # how restore cuts an output: see there
K_MIN, K_MAX = 1, 32                    # the k of knn_points and ball_query, and so the slots of the idx / d2 that group takes
METHODS = ("walk", "grid")              # the neighbour searches of knn_points, chamfer_distance and estimate_normals


def _err(what, msg):
    raise ValueError("%s: %s" % (what, msg))


def _check_k(k, what, lo, hi):
    if isinstance(k, bool) or not isinstance(k, int) or not (lo <= k <= hi):
        _err(what, "k must be an int in [%d, %d], got %r" % (lo, hi, k))


def _check_method(method, what):
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError('%s: method must be "walk" or "grid", got %r' % (what, method))


def _check_deterministic(deterministic, what):
    """deterministic= of knn_points, ball_query and chamfer_distance (group.py's _inverse_arg has the same wording)"""
    if not isinstance(deterministic, bool):
        raise ValueError("%s: deterministic must be True or False, got %r" % (what, deterministic))


def _check_points(t, name, what, min_cols=3):
    if not isinstance(t, torch.Tensor):
        _err(what, "%s must be a tensor, got %s" % (name, type(t).__name__))
    if t.dtype not in _DT:
        _err(what, "%s must be float32 or float64, got %s" % (name, t.dtype))
    if t.dim() < 1 or t.shape[-1] < min_cols:
        _err(what, "%s needs at least %s, got shape %s" % (name, "3 columns (x, y, z)" if min_cols == 3 else "%d column(s)" % min_cols, tuple(t.shape)))


def check(t, rows, what, name="points", rows_name="rows", empty_ok=False, flat_rows=False, min_cols=3):
    """-> (form, batch (N,m,c), rows or None, lengths of a list or None); ValueError for anything invalid.

    empty_ok: clouds without rows are let through (place pads them).  flat_rows: rows may have any shape with N elements, a single cloud
    (N = 1) included; otherwise they are 1-D and need a padded batch.  min_cols: the fewest columns a table may have (3: points; 1: a
    feature table, a per-point weight)."""
    if isinstance(t, (list, tuple)):
        if not t:
            _err(what, "%s is an empty list" % name)
        for i, c in enumerate(t):
            _check_points(c, "%s[%d]" % (name, i), what, min_cols)
            if c.dim() != 2:
                _err(what, "%s[%d] must be (m_b, c), got shape %s" % (name, i, tuple(c.shape)))
        if len({c.shape[1] for c in t}) != 1 or len({c.dtype for c in t}) != 1 or len({c.device for c in t}) != 1:
            _err(what, "the clouds of %s need one column count, dtype and device" % name)
        if rows is not None:
            _err(what, "%s is a list: %s come from the list itself" % (name, rows_name))
        lens = [c.shape[0] for c in t]
        form, batch, rows = "list", torch.nn.utils.rnn.pad_sequence(list(t), batch_first=True), torch.tensor(lens, dtype=torch.int32)
    else:
        _check_points(t, name, what, min_cols)
        if t.dim() not in (2, 3):
            _err(what, "%s must be (m, c), (N, m, c) or a list of (m_b, c), got shape %s" % (name, tuple(t.shape)))
        if t.dim() == 2 and rows is not None and not flat_rows:
            _err(what, "%s needs a padded batch (N, m, c)" % rows_name)
        form, batch, lens = ("single", t.unsqueeze(0), None) if t.dim() == 2 else ("batch", t, None)
    N, m = batch.shape[0], batch.shape[1]
    if N < 1 or (m < 1 and not empty_ok):
        _err(what, "%s is an empty batch, shape %s" % (name, tuple(batch.shape)))
    if lens is None and rows is not None:
        rows = torch.as_tensor(rows)
        if rows.dtype.is_floating_point or rows.dtype.is_complex or rows.dtype == torch.bool or rows.numel() != N \
                or not (flat_rows or rows.dim() == 1):
            _err(what, "%s must be %d integer counts" % (rows_name, N))
        if not rows.is_cuda and (int(rows.min()) < 0 or int(rows.max()) > m):
            _err(what, "%s must lie in [0, %d]" % (rows_name, m))
    return form, batch, rows, lens


def check_pair(x, y, x_rows, y_rows, what, nx="x", ny="y", min_cols=3):
    """check on both arguments of a two-cloud operator (either side may be empty), and that they go together -> (check(x), check(y));
    nx, ny: the arguments' names in the messages"""
    cx = check(x, x_rows, what, nx, "x_rows", empty_ok=True, min_cols=min_cols)
    cy = check(y, y_rows, what, ny, "y_rows", empty_ok=True, min_cols=min_cols)
    bx, by = cx[1], cy[1]
    if cx[0] != cy[0]:
        _err(what, "%s and %s must have the same form (single clouds, padded batches or lists), got %s and %s" % (nx, ny, cx[0], cy[0]))
    if bx.dtype != by.dtype:
        _err(what, "%s and %s must have one dtype, got %s and %s" % (nx, ny, bx.dtype, by.dtype))
    if bx.device != by.device:
        _err(what, "%s and %s must be on one device, got %s and %s" % (nx, ny, bx.device, by.device))
    if bx.shape[0] != by.shape[0]:
        _err(what, "%s and %s must hold the same number of clouds, got %d and %d" % (nx, ny, bx.shape[0], by.shape[0]))
    return cx, cy


_INT = (torch.int32, torch.int64)


def check_slots(t, what, name, like, integer, k_lo, k_hi):
    """An argument with k slots per row -- the idx / d2 that knn_points and ball_query return: (n, k), (N, n, k) or a list of (n_b, k)
    -> (batch (N,n,k), lengths of a list or None); ValueError for anything invalid.

    like: the checked form and batch (form, batch) of the argument it goes with: the same form, cloud count and device.  integer: int32 or
    int64 indices, kept as they are (a list is padded with -1, the empty slot); otherwise the dtype of like's batch (padded with 0)."""
    form, other = like
    is_list = isinstance(t, (list, tuple))
    items = list(t) if is_list else [t]
    if is_list and not items:
        _err(what, "%s is an empty list" % name)
    for i, c in enumerate(items):
        nm = "%s[%d]" % (name, i) if is_list else name
        if not isinstance(c, torch.Tensor):
            _err(what, "%s must be a tensor, got %s" % (nm, type(c).__name__))
        if integer and c.dtype not in _INT:
            _err(what, "%s must be int32 or int64, got %s" % (nm, c.dtype))
        if not integer and c.dtype != other.dtype:
            _err(what, "%s must have the dtype of the features, %s, got %s" % (nm, other.dtype, c.dtype))
        if is_list and c.dim() != 2:
            _err(what, "%s must be (n_b, k), got shape %s" % (nm, tuple(c.shape)))
    if not is_list and t.dim() not in (2, 3):
        _err(what, "%s must be (n, k), (N, n, k) or a list of (n_b, k), got shape %s" % (name, tuple(t.shape)))
    mine = "list" if is_list else ("single" if t.dim() == 2 else "batch")
    if mine != form:
        _err(what, "%s must have the form of the features (single clouds, padded batches or lists), got %s and %s" % (name, mine, form))
    if len({c.shape[-1] for c in items}) != 1 or len({c.dtype for c in items}) != 1 or len({c.device for c in items}) != 1:
        _err(what, "the clouds of %s need one slot count, dtype and device" % name)
    k = items[0].shape[-1]
    if not (k_lo <= k <= k_hi):
        _err(what, "%s must have k in [%d, %d] slots, got shape %s" % (name, k_lo, k_hi, tuple(items[0].shape)))
    if items[0].device != other.device:
        _err(what, "%s and the features must be on one device, got %s and %s" % (name, items[0].device, other.device))
    if is_list:
        batch, lens = torch.nn.utils.rnn.pad_sequence(items, batch_first=True, padding_value=-1 if integer else 0), [c.shape[0] for c in items]
    else:
        batch, lens = (t.unsqueeze(0) if t.dim() == 2 else t), None
    if batch.shape[0] != other.shape[0]:
        _err(what, "%s and the features must hold the same number of clouds, got %d and %d" % (name, batch.shape[0], other.shape[0]))
    if batch.shape[1] < 1:
        _err(what, "%s has no rows, shape %s" % (name, tuple(batch.shape)))
    return batch, lens


def check_mask(t, what, name, like):
    """A keep-mask, one torch.bool per row, in the form of the points it goes with: (m,), (N, m) or a list of (m_b,) -> batch (N, m) bool
    (a list is padded with False); ValueError for anything invalid.

    like: the checked form, batch and list lengths (form, batch, lens) of the points: the same form, cloud count, row counts and device."""
    form, other, lens = like
    is_list = isinstance(t, (list, tuple))
    items = list(t) if is_list else [t]
    if is_list and not items:
        _err(what, "%s is an empty list" % name)
    for i, c in enumerate(items):
        nm = "%s[%d]" % (name, i) if is_list else name
        if not isinstance(c, torch.Tensor):
            _err(what, "%s must be a tensor, got %s" % (nm, type(c).__name__))
        if c.dtype != torch.bool:
            _err(what, "%s must be torch.bool, got %s" % (nm, c.dtype))
        if is_list and c.dim() != 1:
            _err(what, "%s must be (m_b,), got shape %s" % (nm, tuple(c.shape)))
        if c.device != other.device:
            _err(what, "%s and the points must be on one device, got %s and %s" % (nm, c.device, other.device))
    if not is_list and t.dim() not in (1, 2):
        _err(what, "%s must be (m,), (N, m) or a list of (m_b,), got shape %s" % (name, tuple(t.shape)))
    mine = "list" if is_list else ("single" if t.dim() == 1 else "batch")
    if mine != form:
        _err(what, "%s must have the form of the points (single clouds, padded batches or lists), got %s and %s" % (name, mine, form))
    if is_list:
        if [c.shape[0] for c in items] != list(lens):
            _err(what, "%s must hold one entry per row of every cloud, got lengths %s for clouds of %s rows" % (name, [c.shape[0] for c in items], list(lens)))
        return torch.nn.utils.rnn.pad_sequence(items, batch_first=True, padding_value=False)
    batch = t.unsqueeze(0) if t.dim() == 1 else t
    if tuple(batch.shape) != tuple(other.shape[:2]):
        _err(what, "%s must hold one entry per row, shape %s, got %s" % (name, tuple(other.shape[1:2] if form == "single" else other.shape[:2]), tuple(t.shape)))
    return batch


def check_table(t, what, name, like, cols):
    """A table with one row of exactly `cols` values per point -- normals -- in the form of the points it goes with: (m, cols), (N, m, cols)
    or a list of (m_b, cols) -> batch (N, m, cols) (a list is padded with 0); ValueError for anything invalid.

    like: the checked form, batch and list lengths (form, batch, lens) of the points: the same form, dtype, device, cloud and row counts."""
    form, other, lens = like
    is_list = isinstance(t, (list, tuple))
    items = list(t) if is_list else [t]
    if is_list and not items:
        _err(what, "%s is an empty list" % name)
    for i, c in enumerate(items):
        nm = "%s[%d]" % (name, i) if is_list else name
        if not isinstance(c, torch.Tensor):
            _err(what, "%s must be a tensor, got %s" % (nm, type(c).__name__))
        if c.dtype != other.dtype:
            _err(what, "%s must have the dtype of the points, %s, got %s" % (nm, other.dtype, c.dtype))
        if c.device != other.device:
            _err(what, "%s and the points must be on one device, got %s and %s" % (nm, c.device, other.device))
        if (is_list and c.dim() != 2) or c.dim() < 1 or c.shape[-1] != cols:
            _err(what, "%s must have %d columns per row, got shape %s" % (nm, cols, tuple(c.shape)))
    if not is_list and t.dim() not in (2, 3):
        _err(what, "%s must be (m, %d), (N, m, %d) or a list of (m_b, %d), got shape %s" % (name, cols, cols, cols, tuple(t.shape)))
    mine = "list" if is_list else ("single" if t.dim() == 2 else "batch")
    if mine != form:
        _err(what, "%s must have the form of the points (single clouds, padded batches or lists), got %s and %s" % (name, mine, form))
    if is_list:
        if [c.shape[0] for c in items] != list(lens):
            _err(what, "%s must hold one row per point of every cloud, got lengths %s for clouds of %s rows" % (name, [c.shape[0] for c in items], list(lens)))
        return torch.nn.utils.rnn.pad_sequence(items, batch_first=True)
    batch = t.unsqueeze(0) if t.dim() == 2 else t
    if tuple(batch.shape[:2]) != tuple(other.shape[:2]):
        _err(what, "%s must hold one row per point, shape %s, got %s" % (name, tuple(other.shape[1:2] if form == "single" else other.shape[:2]) + (cols,), tuple(t.shape)))
    return batch


def place(batch, rows, xyz=False):
    """A checked batch and its rows on the compute device -> (on_cpu, batch (N,m',c') contiguous, rows (N,) int32 or None).

    xyz: only columns 0:3 go to the library unless there are 3 or 6.  A batch without rows is padded to one row with a row count of 0."""
    on_cpu = not batch.is_cuda
    dev = compute_device() if on_cpu else batch.device
    b = batch.to(dev)
    if xyz and b.shape[2] not in (3, 6):
        b = b[..., :3]
    if b.shape[1] == 0:                                     # the library needs a row: one pad row, no row taking part
        b = torch.zeros((b.shape[0], 1, b.shape[2]), dtype=b.dtype, device=dev) + b.sum() * 0
        rows = torch.zeros(b.shape[0], dtype=torch.int32)
    if rows is not None:
        rows = rows.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    return on_cpu, b.contiguous(), rows


def pair(x, y, x_rows, y_rows, what):
    """check_pair, then place with xyz on both -> (form, on_cpu, lens_x, n, m, x (N,n',c), y (N,m',c), x_rows, y_rows) with n', m' >= 1"""
    (form, bx, rx, lx), (_, by, ry, _) = check_pair(x, y, x_rows, y_rows, what)
    on_cpu, bx_d, rx_d = place(bx, rx, xyz=True)
    _, by_d, ry_d = place(by, ry, xyz=True)
    return form, on_cpu, lx, bx.shape[1], by.shape[1], bx_d, by_d, rx_d, ry_d


def pair_features(x, y, x_rows, y_rows, what, d_max):
    """pair for two descriptor tables (match.py): every column takes part (1 <= D <= d_max, the same D on both sides) -> pair's tuple"""
    (form, bx, rx, lx), (_, by, ry, _) = check_pair(x, y, x_rows, y_rows, what, "fx", "fy", min_cols=1)
    if bx.shape[2] != by.shape[2] or bx.shape[2] > d_max:
        _err(what, "fx and fy need the same number of channels D in [1, %d], got %d and %d" % (d_max, bx.shape[2], by.shape[2]))
    on_cpu, bx_d, rx_d = place(bx, rx)
    _, by_d, ry_d = place(by, ry)
    return form, on_cpu, lx, bx.shape[1], by.shape[1], bx_d, by_d, rx_d, ry_d


def restore(form, on_cpu, n, lens, outs, k=None, voxels=None):
    """The library's results in the caller's form, on the caller's device -> a tuple with one entry per output.

    outs: [(kind, tensor (N, ...))].  ROW: one entry per input row, cut to the cloud's n / lens[b] rows; SLOT: k slots, a list's cut to
    min(k, lens[b]); CLOUD: one value per cloud; VOXEL: one entry per voxel, cut to voxels[b].  A single cloud gets cloud 0 of each, a
    list one tensor per cloud, a batch the tensors themselves."""
    if on_cpu:
        outs = [(kind, t.cpu()) for kind, t in outs]

    def cut(kind, t, b, rows):
        if kind == CLOUD:
            return t[b]
        if kind == SLOT:
            return t[b, :min(k, rows)] if form == "list" else t[b]
        return t[b, :(rows if kind == ROW else int(voxels[b]))]
    if form == "list":
        return tuple([cut(kind, t, b, lens[b]) for b in range(len(lens))] for kind, t in outs)
    if form == "single":
        return tuple(cut(kind, t, 0, n) for kind, t in outs)
    return tuple(t[:, :n] if kind == ROW and t.shape[1] != n else t for kind, t in outs)
