"""numpy restatement of dicp_amd.ball.ball_query for one pair of clouds: brute force in the clouds' dtype, stable (d2, index) order.

The variants (`strict`, `drop`) are wrong on purpose: the tests use them to show that their comparison tells them from the definition."""
import numpy as np


def d2_matrix(x, y):
    """(n, m) squared distances as the kernels round them: (xx + yy) + zz with dx = y.x - x.x, every operation rounded in the dtype"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        dx = y[None, :, 0] - x[:, None, 0]
        dy = y[None, :, 1] - x[:, None, 1]
        dz = y[None, :, 2] - x[:, None, 2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        return (xx + yy) + zz


def r2_of(radius, dtype):
    r = np.asarray(radius, dtype=dtype)
    with np.errstate(over="ignore", under="ignore"):
        return r * r


def ball_ref(x, y, radius, k, x_rows=None, y_rows=None, strict=False, drop=None):
    """x (n, c), y (m, c) of one dtype -> d2 (n, k), idx (n, k) int64, counts (n,) int32.

    strict: `<` in place of `<=`.  drop = (i, s): query i loses its s-th nearest candidate."""
    dtype = x.dtype
    assert y.dtype == dtype
    n, m = x.shape[0], y.shape[0]
    nb = n if x_rows is None else int(x_rows)
    mb = m if y_rows is None else int(y_rows)
    r2 = r2_of(radius, dtype)
    d2 = np.full((n, k), np.inf, dtype=dtype)
    idx = np.full((n, k), -1, dtype=np.int64)
    counts = np.zeros(n, dtype=np.int32)
    if nb == 0 or mb == 0:
        return d2, idx, counts
    D = d2_matrix(x[:nb, :3], y[:mb, :3])
    assert D.dtype == dtype
    with np.errstate(invalid="ignore"):
        cand = np.isfinite(D) & ((D < r2) if strict else (D <= r2))
    cand &= np.isfinite(x[:nb, :3]).all(1)[:, None]
    for i in np.flatnonzero(cand.any(1)):
        j = np.flatnonzero(cand[i])
        j = j[np.argsort(D[i, j], kind="stable")]           # (j ascending and the sort stable: ties by index)
        if drop is not None and drop[0] == i:
            j = np.delete(j, drop[1])
        counts[i] = j.size
        t = min(k, j.size)
        d2[i, :t] = D[i, j[:t]]
        idx[i, :t] = j[:t]
    return d2, idx, counts


def same(got, ref):
    """index for index, d2 bit for bit, counts exactly -> None, or a description of the first difference"""
    for name, a, b in zip(("idx", "d2", "counts"), (got[1], got[0], got[2]), (ref[1], ref[0], ref[2])):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype != b.dtype or a.shape != b.shape:
            return "%s: %s %s against %s %s" % (name, a.dtype, a.shape, b.dtype, b.shape)
        if a.tobytes() != b.tobytes():
            w = np.argwhere(a != b)
            return "%s differs at %s: %r against %r" % (name, w[0] if len(w) else "?", a[tuple(w[0])] if len(w) else None, b[tuple(w[0])] if len(w) else None)
    return None
