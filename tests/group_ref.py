"""The definition of dicp_amd.group in numpy, for one cloud: a feature table f (m, C), indices idx (n, k), optionally rows (the live rows of f).

Every function restates a docstring of dicp_amd/group.py with one numpy operation per rounding, in the table's dtype T, looping over the k
slots in slot order.  interp_exact / gd2_exact evaluate the same expressions in float64 on the same inputs and return the sums that the
error bounds are made of.  A plain module (no fixtures): the tests put this directory on sys.path and import it.
"""
import numpy as np


def live_slots(idx, m, rows=None):
    """(n, k) bool: 0 <= idx < rows (m without rows)"""
    lim = m if rows is None else min(max(int(rows), 0), m)
    return (idx >= 0) & (idx < lim)


def _rows_of(f, idx, live):
    """f[idx] with the empty slots reading row 0 (masked by the caller) -> (n, k, C)"""
    return f[np.where(live, idx, 0)]


def group_ref(f, idx, rows=None, centers=None):
    """-> (n, k, C): f[idx] on live slots (columns 0:Cc minus centers, one rounding), 0 on empty ones"""
    live = live_slots(idx, f.shape[0], rows)
    out = _rows_of(f, idx, live).copy()
    if centers is not None:
        cc = centers.shape[1]
        out[:, :, :cc] = out[:, :, :cc] - centers[:, None, :]
    out[~live] = 0
    return out


def _interp_weights(idx, d2, eps, m, rows, T):
    """live (n, k), r (n, k), R (n,), w (n, k) in dtype T, slot order"""
    live = live_slots(idx, m, rows) & np.isfinite(d2)
    d = np.where(live, d2, 0).astype(T)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(live, T(1) / (d + T(eps)), T(0)).astype(T)
        R = np.zeros(idx.shape[0], dtype=T)
        for s in range(idx.shape[1]):
            R = (R + r[:, s]).astype(T)
        w = np.where(R[:, None] > 0, r / np.where(R > 0, R, T(1))[:, None], T(0)).astype(T)
    return live, r, R, w


def interp_ref(f, idx, d2, eps, rows=None):
    """-> (n, C) in f's dtype: sum_s w_s f[idx_s], separate roundings, slot order; 0 without a live slot"""
    T = f.dtype.type
    live, r, R, w = _interp_weights(idx, d2, T(eps), f.shape[0], rows, T)
    x = _rows_of(f, idx, live)
    out = np.zeros((idx.shape[0], f.shape[1]), dtype=T)
    for s in range(idx.shape[1]):
        p = (w[:, s, None] * x[:, s]).astype(T)
        out = np.where(live[:, s, None], (out + p).astype(T), out)
    return out


def interp_exact(f, idx, d2, eps, rows=None):
    """The same expression in float64 on the same inputs (eps rounded to f's dtype first) -> (out (n, C), scale (n, C) = sum_s w_s |f[idx_s]|)"""
    eps = float(f.dtype.type(eps))
    live, r, R, w = _interp_weights(idx, d2.astype(np.float64), eps, f.shape[0], rows, np.float64)
    x = _rows_of(f.astype(np.float64), idx, live)
    wl = np.where(live, w, 0.0)
    return (wl[:, :, None] * x).sum(1), (wl[:, :, None] * np.abs(x)).sum(1)


def interp_bound(k, dtype):
    """the factor of scale in the forward's bound: (2k + 8) u"""
    return (2 * k + 8) * float(np.finfo(dtype).eps) / 2


def gd2_ref(f, idx, d2, eps, g, rows=None):
    """g_d2 (n, k) in f's dtype: -(r_s^2 / R) sum_c g_c (f[idx_s, c] - out_c), separate roundings, channels in order; 0 on empty slots"""
    T = f.dtype.type
    live, r, R, w = _interp_weights(idx, d2, T(eps), f.shape[0], rows, T)
    out = interp_ref(f, idx, d2, eps, rows)
    x = _rows_of(f, idx, live)
    n, k = idx.shape
    dot = np.zeros((n, k), dtype=T)
    for c in range(f.shape[1]):
        dd = (x[:, :, c] - out[:, None, c]).astype(T)
        dot = (dot + (g[:, None, c] * dd).astype(T)).astype(T)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = ((r * r).astype(T) / np.where(R > 0, R, T(1))[:, None]).astype(T)
    return np.where(live, -(q * dot), T(0)).astype(T)


def gd2_exact(f, idx, d2, eps, g, rows=None):
    """float64 on the same inputs -> (g_d2 (n, k), scale (n, k) = (r_s^2 / R) sum_c |g_c| (|f_sc| + sum_t w_t |f_tc|))"""
    eps = float(f.dtype.type(eps))
    live, r, R, w = _interp_weights(idx, d2.astype(np.float64), eps, f.shape[0], rows, np.float64)
    x = _rows_of(f.astype(np.float64), idx, live)
    out, scale = interp_exact(f, idx, d2, eps, rows)
    g = g.astype(np.float64)
    dot = ((x - out[:, None, :]) * g[:, None, :]).sum(2)
    mag = ((np.abs(x) + scale[:, None, :]) * np.abs(g)[:, None, :]).sum(2)
    q = r * r / np.where(R > 0, R, 1.0)[:, None]
    return np.where(live, -q * dot, 0.0), np.where(live, q * mag, 0.0)


def gd2_bound(k, C, dtype, widen=0):
    """the factor of scale in g_d2's bound: (C + 3k + 16 + widen) u"""
    return (C + 3 * k + 16 + widen) * float(np.finfo(dtype).eps) / 2


def ulp_apart(a, b):
    """the largest distance in units in the last place between two arrays of one float dtype (finite, same sign pattern expected)"""
    it = {np.dtype(np.float32): np.int32, np.dtype(np.float64): np.int64}[a.dtype]
    ia, ib = a.view(it).astype(np.int64), b.view(it).astype(np.int64)
    return int(np.abs(ia - ib).max()) if a.size else 0


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ test inputs
def make_idx(n, k, m, rows, seed, dtype=np.int64):
    """(n, k) indices holding every kind of slot: live rows, -1, other negatives, exactly rows, rows..m-1, >= m; queries that are wholly
    empty (every 5th), full (every 5th + 1) and partly full (the rest, live slots not only leading).  rows <= m."""
    rng = np.random.default_rng(seed)
    lim = max(int(rows), 1)
    idx = rng.integers(0, lim, size=(n, k))
    kind = rng.integers(0, 8, size=(n, k))
    idx = np.where(kind == 0, -1, idx)
    idx = np.where(kind == 1, -rng.integers(2, 2 ** 31 - 1, size=(n, k)), idx)
    idx = np.where(kind == 2, rows, idx)
    idx = np.where(kind == 3, m + rng.integers(0, 2 ** 31 - 1 - m, size=(n, k)), idx)
    q = np.arange(n)
    full = rng.integers(0, lim, size=(n, k))
    idx = np.where((q % 5 == 1)[:, None], full, idx)
    empty = np.where(rng.integers(0, 2, size=(n, k)) == 0, -1, rows)
    idx = np.where((q % 5 == 0)[:, None], empty, idx)
    if rows == 0:
        idx = np.where(idx == 0, -1, idx)
    return idx.astype(dtype)


def idx_kinds(idx, m, rows):
    """what make_idx promises, for the tests to assert"""
    live = live_slots(idx, m, rows)
    per = live.sum(1)
    k = idx.shape[1]
    return {"empty_query": bool((per == 0).any()), "full_query": bool((per == k).any()), "partial_query": bool(((per > 0) & (per < k)).any()) or k == 1,
            "minus_one": bool((idx == -1).any()), "other_negative": bool((idx < -1).any()), "at_rows": bool((idx == rows).any()),
            "past_m": bool((idx >= m).any())}


def make_d2(n, k, seed, dtype, near=False):
    """(n, k) squared distances >= 0: eight decades with exact zeros (some queries with several), a few +inf; near: within a factor of 4"""
    rng = np.random.default_rng(seed)
    if near:
        return (0.5 + 1.5 * rng.random((n, k))).astype(dtype)
    d = 10.0 ** rng.uniform(-6, 2, size=(n, k))
    d = np.where(rng.integers(0, 6, size=(n, k)) == 0, 0.0, d)
    d = np.where(rng.integers(0, 12, size=(n, k)) == 0, np.inf, d)
    return d.astype(dtype)
