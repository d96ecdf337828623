"""The definition of dicp_amd.match (knn_features, match_features and the gradient of d2) in numpy, for one cloud.

fma is the correctly rounded fused multiply-add.  float32: the product of two float32 is exact in float64 (48 bits); c is added with a
TwoSum, the float64 sum is rounded to ODD when the TwoSum error is non-zero, and the cast to float32 then rounds once (float64 keeps more
than 2 * 24 + 2 bits, so round-to-odd followed by round-to-nearest is round-to-nearest of the exact value; float32(float64(a) * b + c)
alone rounds twice).  float64: exact rational arithmetic (fractions) per element -- for the small shapes of the tests.  Everything else is
one numpy operation per rounding in the tables' dtype T.  The `wrong` keyword makes the deliberately wrong restatements that the tests show
the comparison to refuse.  A plain module (no fixtures): the tests put this directory on sys.path and import it.
"""
from fractions import Fraction

import numpy as np

DET_CHUNK = 64
WRONG = ("unfused", "descending", "h_last", "tie_high", "d2_from_score")


def fma32(a, b, c):
    """elementwise fmaf on float32 arrays (broadcast) -> float32"""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)         # exact
        cd = c.astype(np.float64)
        s = p + cd
        bb = s - p
        err = (p - (s - bb)) + (cd - bb)                        # TwoSum: p + c = s + err exactly (finite s)
        odd = (s.view(np.int64) & 1) != 0
        fix = np.isfinite(s) & (err != 0) & ~odd
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def _fma64_one(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return a * b + c                                        # (the product is then -c exactly: the float sum has the sign of the fma's zero)
    try:
        return float(r)                                         # correctly rounded
    except OverflowError:
        return float("inf") if r > 0 else float("-inf")


_fma64_vec = np.frompyfunc(_fma64_one, 3, 1)


def fma64(a, b, c):
    return _fma64_vec(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64)).astype(np.float64)


def fma(a, b, c, dtype):
    return fma32(a, b, c) if np.dtype(dtype) == np.float32 else fma64(a, b, c)


def half_norm(y, wrong=None):
    """(m, D) -> (m,): h_j"""
    T = y.dtype.type
    q = np.zeros(y.shape[0], dtype=y.dtype)
    with np.errstate(all="ignore"):
        for c in range(y.shape[1]):
            q = (q + (y[:, c] * y[:, c]).astype(T)).astype(T) if wrong == "unfused" else fma(y[:, c], y[:, c], q, T)
        return (T(0.5) * q).astype(T)


def scores(x, y, wrong=None):
    """(n, D), (m, D) -> (n, m): score(i, j)"""
    T = x.dtype.type
    n, D = x.shape
    h = half_norm(y, wrong)
    s = np.broadcast_to(h[None, :], (n, y.shape[0])).astype(T)
    if wrong == "h_last":
        s = np.zeros_like(s)
    order = range(D - 1, -1, -1) if wrong == "descending" else range(D)
    with np.errstate(all="ignore"):
        for c in order:
            if wrong == "unfused":
                s = (s + ((-x[:, c, None]) * y[None, :, c]).astype(T)).astype(T)
            else:
                s = fma(-x[:, c, None], y[None, :, c], s, T)
        if wrong == "h_last":
            s = (s + h[None, :]).astype(T)
    return s


def refine(x, yj):
    """x (..., D), yj (..., D) -> (...): the d2 of the definition"""
    T = x.dtype.type
    r = np.zeros(np.broadcast(x[..., 0], yj[..., 0]).shape, dtype=x.dtype)
    with np.errstate(all="ignore"):
        for c in range(x.shape[-1]):
            t = (x[..., c] - yj[..., c]).astype(T)
            r = fma(t, t, r, T)
    return r


def knn_features_ref(x, y, k, x_rows=None, y_rows=None, wrong=None, return_scores=False):
    """-> d2 (n, k) T, idx (n, k) int64 of one cloud"""
    T = x.dtype.type
    n, m = x.shape[0], y.shape[0]
    xr = n if x_rows is None else int(x_rows)
    yr = m if y_rows is None else int(y_rows)
    d2 = np.full((n, k), np.inf, dtype=x.dtype)
    idx = np.full((n, k), -1, dtype=np.int64)
    sc = np.full((n, k), np.inf, dtype=x.dtype)
    if xr and yr:
        s = scores(x[:xr], y[:yr], wrong)
        for i in range(xr):
            cand = np.flatnonzero(np.isfinite(s[i]))
            key_j = -cand if wrong == "tie_high" else cand
            order = cand[np.lexsort((key_j, s[i, cand]))][:k]
            idx[i, :order.size] = order
            sc[i, :order.size] = s[i, order]
            if order.size:
                d2[i, :order.size] = refine(x[i][None, :], y[order])
            if wrong == "d2_from_score":                        # |x - y|^2 = 2 score + |x|^2
                xx = (x[i].astype(T) * x[i]).sum(dtype=T)
                d2[i, :order.size] = (T(2) * s[i, order] + xx).astype(T)
    return (d2, idx, sc) if return_scores else (d2, idx)


def match_features_ref(x, y, x_rows=None, y_rows=None, mutual=True, ratio=None, max_d2=None):
    """-> idx (n,) int64, d2 (n,) T of one cloud"""
    T = x.dtype.type
    d2, idx = knn_features_ref(x, y, 1 if ratio is None else 2, x_rows, y_rows)
    keep = idx[:, 0] >= 0
    with np.errstate(all="ignore"):
        if ratio is not None:
            keep &= d2[:, 0] <= (T(float(ratio) * float(ratio)) * d2[:, 1]).astype(T)
        if max_d2 is not None:
            keep &= d2[:, 0] <= T(max_d2)
    if mutual:
        _, back = knn_features_ref(y, x, 1, y_rows, x_rows)
        keep &= back[np.clip(idx[:, 0], 0, None), 0] == np.arange(x.shape[0])
    return np.where(keep, idx[:, 0], -1), np.where(keep, d2[:, 0], np.inf).astype(x.dtype)


# ------------------------------------------------------------------ the gradient
def term(g, xc, yc, T):
    """t_c of the definition, rounded once"""
    with np.errstate(all="ignore"):
        return ((2.0 * np.float64(g)) * (np.asarray(xc, dtype=np.float64) - np.asarray(yc, dtype=np.float64))).astype(T)


def grad_x_ref(g, idx, x, y):
    """-> (n, D): the sum of the query's terms in slot order from +0"""
    T = x.dtype.type
    out = np.zeros_like(x)
    with np.errstate(all="ignore"):
        for i in range(x.shape[0]):
            for s in range(idx.shape[1]):
                j = idx[i, s]
                if j < 0 or j >= y.shape[0] or g[i, s] == 0:
                    continue
                out[i] = (out[i] + term(g[i, s], x[i], y[j], T)).astype(T)
    return out


def invert(idx, m, rows=None):
    """offsets (m + 1,), slots (n k,) of group.invert_neighbors for one cloud"""
    lim = m if rows is None else min(max(int(rows), 0), m)
    row = np.where((idx >= 0) & (idx < lim), idx, -1).reshape(-1)
    q = np.flatnonzero(row >= 0)
    order = q[np.argsort(row[q], kind="stable")]
    slots = np.full(row.size, -1, dtype=np.int32)
    slots[:order.size] = order
    offsets = np.zeros(m + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(np.bincount(row[q], minlength=m)[:m])
    return offsets, slots


def grad_y_det_ref(g, idx, x, y, rows=None, chunk=DET_CHUNK, wrong=None):
    """-> (m, D): the deterministic gradient of fy.  wrong: "descending" walks every list backwards, "one_chunk" ignores the chunks"""
    T = x.dtype.type
    m, k = y.shape[0], idx.shape[1]
    offsets, slots = invert(idx, m, rows)
    out = np.zeros_like(y)
    gf = g.reshape(-1)
    with np.errstate(all="ignore"):
        for j in range(m if rows is None else min(int(rows), m)):
            lst = slots[offsets[j]:offsets[j + 1]]
            if wrong == "descending":
                lst = lst[::-1]
            total, part = np.zeros(y.shape[1], dtype=T), np.zeros(y.shape[1], dtype=T)
            for e, q in enumerate(lst):
                if e > 0 and e % chunk == 0 and wrong != "one_chunk":
                    total = (total + part).astype(T)
                    part = np.zeros(y.shape[1], dtype=T)
                if gf[q] == 0:
                    continue
                part = (part + (-term(gf[q], x[q // k], y[j], T))).astype(T)
            out[j] = part if (len(lst) <= chunk or wrong == "one_chunk") else (total + part).astype(T)
    return out
