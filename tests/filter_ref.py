"""numpy / plain-Python restatement of the three definitions of dicp_amd/filter.py, for the CPU and GPU tests: the stable compaction with
index and pos, sum64 as explicit loops, and the statistical filter's slot rule, mean distances, statistics and decision.

Python floats are IEEE doubles and math.sqrt is correctly rounded, so every operation below rounds once, in the order written.
The keyword switches of sum64 / outlier_ref state WRONG rules; the tests use them to find data on which a wrong rule shows."""
import math
from fractions import Fraction

import numpy as np

CHUNK = 64


def select_ref(points, mask, rows=None):
    """points (m, c), mask (m,) bool -> out (m, c), rows_out, index (m,) int64, pos (m,) int32"""
    m = points.shape[0]
    mb = m if rows is None else int(rows)
    keep = np.asarray(mask, dtype=bool).copy()
    keep[mb:] = False
    src = np.flatnonzero(keep)
    out = np.zeros_like(points)
    out[:src.size] = points[src]
    index = np.full(m, -1, dtype=np.int64)
    index[:src.size] = src
    pos = np.full(m, -1, dtype=np.int32)
    pos[src] = np.arange(src.size, dtype=np.int32)
    return out, int(src.size), index, pos


def select_grad_ref(g_out, pos):
    """the gradient of select_ref's out: g_out (m, c) -> (m, c)"""
    g = np.zeros_like(g_out)
    kept = pos >= 0
    g[kept] = g_out[pos[kept]]
    return g


def _sequential(values):
    s = 0.0
    for v in values:
        s = s + v
    return s


def sum64(values, tree=True):
    """tree=False: the plain sequential sum (a wrong rule)"""
    v = [float(x) for x in values]
    if not tree:
        return _sequential(v)
    while len(v) > CHUNK:
        v = [_sequential(v[j:j + CHUNK]) for j in range(0, len(v), CHUNK)]
    return _sequential(v)


def row_mean(d2, idx, i, k, skip_self=True):
    """row i's k + 1 slots -> (md, cnt)"""
    s, cnt = 0.0, 0
    for q in range(k + 1):
        j = int(idx[q])
        if j < 0 or (skip_self and j == i):
            continue
        if cnt == k:
            break
        s = s + math.sqrt(float(d2[q]))
        cnt += 1
    return (s / cnt if cnt else math.inf), cnt


def _fma(a, b, c):
    """a b + c rounded once (exact rational arithmetic; int / int rounds correctly)"""
    f = Fraction(a) * Fraction(b) + Fraction(c)
    return f.numerator / f.denominator


def outlier_ref(d2, idx, k, std_ratio, rows=None, tree=True, population=False, strict=False, skip_self=True, fused=False):
    """d2 (m, k + 1), idx (m, k + 1) -> md (m,) float64, stats (3,) float64 = mean, std, thr, mask (m,) bool

    tree / population / strict / skip_self / fused: wrong rules -- plain sequential sums, a variance over V, `<` for `<=`, a self slot
    that counts, each chunk's squares fused into its additions."""
    m = d2.shape[0]
    mb = m if rows is None else int(rows)
    md = np.full(m, np.inf, dtype=np.float64)
    cnt = np.zeros(m, dtype=np.int64)
    for i in range(mb):
        md[i], cnt[i] = row_mean(d2[i], idx[i], i, k, skip_self)
    vals = [float(x) for x in md[cnt > 0]]
    V = len(vals)
    mean = sum64(vals, tree) / V if V else math.nan
    sq = []
    for x in vals:
        t = x - mean
        sq.append(t * t)
    if fused:                                               # the partials of the first round, each from +0 by fused steps
        sq = []
        for j in range(0, V, CHUNK):
            s = 0.0
            for x in vals[j:j + CHUNK]:
                t = x - mean
                s = _fma(t, t, s)
            sq.append(s)
    std = math.sqrt(sum64(sq, tree) / (V if population else V - 1)) if V >= 2 else 0.0
    p = float(std_ratio) * std
    thr = mean + p
    mask = (cnt > 0) & ((md < thr) if strict else (md <= thr))
    return md, np.array([mean, std, thr], dtype=np.float64), mask


def same_bits(a, b):
    """equal shapes, dtypes and bytes (-0 differs from +0); a NaN equals any NaN at the same place: 0 / 0 has no one bit pattern"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        if not np.array_equal(na, nb):
            return False
        a, b = np.where(na, 0, a), np.where(nb, 0, b)
    return a.tobytes() == b.tobytes()
