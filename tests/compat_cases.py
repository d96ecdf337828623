"""What the CPU and the GPU tests of correspondence_compatibility / prune_correspondences share: the ctypes front of the g++ build of
csrc/dicp_compat.h, the designed edge tables, the random clouds, and the bound of the float64 check of the decisions.

THE BOUND OF A DECISION.  The relation compares e = a - b with thr, a = sqrt(A), b = sqrt(B), A and B one fma chain of three squares of
differences each.  To first order in u (2^-24 for float32, 2^-53 for float64), with the inputs taken as exact: a difference t_a carries a
relative error u, so t_a^2 carries 2 u, and each of the three fma adds u to the partial sum: A carries at most 2 u + 3 u = 5 u relative, its
square root half of that plus its own rounding, 3.5 u a <= 4 u a.  Likewise b.  The subtraction adds u |e|.  So
    |e - e_64| <= 4 u (a + b) + u |e|                                                           (safety factor 1)
and a pair whose float64 margin | |e_64| - tau | exceeds this bound must get the same decision in T and in float64.  The threshold itself is
rounded to T: tau is chosen exactly representable in both dtypes where the check runs, or the rounding u tau is far below the margin of
every qualifying pair.  With coordinates of order 10 and tau = 0.05 the bound is about 4 2^-24 30 = 7e-6 = 1.4e-4 tau in float32: at least
99 % of the pairs of a random cloud qualify, which the tests assert as a condition on their inputs.

A plain module (no fixtures): the tests put this directory on sys.path and import it.
"""
import ctypes

import numpy as np

import hostbuild
import ransac_ref as rr
from ransac_cases import SFX, _ptr, same_bits  # noqa: F401

P_, I, F64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
TAU = 0.05
MIN_QUALIFY = 0.99
RANSAC_SEED = 0         # of the recovery case: chosen on the CPU, where tests/test_compat_host.py shows that with it RANSAC at H = 64 finds the
#                         motion from the pruned matches of all five cases and from the unpruned matches of none


def build():
    lib = hostbuild.build("compat_check.cpp", "compat_check", ("-Wall",))
    lib.cc_iter_max.restype, lib.cc_iter_max.argtypes = I, []
    for s in SFX.values():
        getattr(lib, "cc_relation_" + s).restype = None
        getattr(lib, "cc_relation_" + s).argtypes = [P_, I, F64, F64, P_, P_, P_, P_]
        getattr(lib, "cc_scores_" + s).restype = None
        getattr(lib, "cc_scores_" + s).argtypes = [P_, I, I, F64, F64, P_, P_, P_]
        getattr(lib, "cc_rank_" + s).restype = None
        getattr(lib, "cc_rank_" + s).argtypes = [P_, I, P_]
    return lib


def header_relation(lib, pairs, threshold, min_length=0.0):
    """-> A, B, e (P, P) T and rel (P, P) bool of one cloud's packed pairs, the diagonal included"""
    pairs = np.ascontiguousarray(pairs)
    P = pairs.shape[0]
    A, B, e = (np.empty((P, P), pairs.dtype) for _ in range(3))
    rel = np.empty((P, P), np.uint8)
    getattr(lib, "cc_relation_" + SFX[pairs.dtype.type])(_ptr(pairs), P, float(threshold), float(min_length), _ptr(A), _ptr(B), _ptr(e), _ptr(rel))
    return A, B, e, rel.astype(bool)


def header_scores(lib, pairs, iterations, threshold, min_length=0.0):
    """-> degree (P,) int32, w and v (iterations, P) T"""
    pairs = np.ascontiguousarray(pairs)
    P = pairs.shape[0]
    deg = np.empty(P, np.int32)
    w, v = np.empty((iterations, P), pairs.dtype), np.empty((iterations, P), pairs.dtype)
    getattr(lib, "cc_scores_" + SFX[pairs.dtype.type])(_ptr(pairs), P, int(iterations), float(threshold), float(min_length), _ptr(deg), _ptr(w), _ptr(v))
    return deg, w, v


def header_rank(lib, score):
    score = np.ascontiguousarray(score)
    rank = np.empty(score.shape[0], np.int32)
    getattr(lib, "cc_rank_" + SFX[score.dtype.type])(_ptr(score), score.shape[0], _ptr(rank))
    return rank


# ------------------------------------------------------------------ designed tables
def _table(name, x, y, dtype, threshold, min_length=0.0, idx=None):
    x, y = np.asarray(x, dtype=dtype).reshape(-1, 3), np.asarray(y, dtype=dtype).reshape(-1, 3)
    idx = np.arange(x.shape[0], dtype=np.int64) if idx is None else np.asarray(idx, dtype=np.int64)
    return dict(name=name, x=x, y=y, idx=idx, threshold=threshold, min_length=min_length)


def edge_tables(dtype):
    """The exact edges as small clouds of matches (idx the identity unless said otherwise).  The tests state what each must give."""
    T = dtype
    one, half = T(1), T(0.5)
    up, dn = np.nextafter(one, T(2)), np.nextafter(one, T(0))
    out = []
    # lattice points: every length is exact.  From match 0: a = 5, 13, 5, 10 and b = 4, 12, 7, 10: e = 1, 1, -2, 0 against threshold 1
    out.append(_table("lattice", [(0, 0, 0), (3, 4, 0), (5, 12, 0), (0, 3, 4), (6, 8, 0)], [(0, 0, 0), (0, 0, 4), (0, 12, 0), (7, 0, 0), (0, 6, 8)], T, 1.0))
    # on one axis sqrt(fma(d, d, 0)) = d exactly: from match 0, e = 1 + ulp (out), 1 (in), 1 - ulp/2 = the next number below 1 (in)
    out.append(_table("one_ulp", [(0, 0, 0), (half + up, 0, 0), (0, 1.5, 0), (0, 0, 1.5)], [(0, 0, 0), (half, 0, 0), (0, half, 0), (0, 0, T(1.5) - dn)], T, 1.0))
    # a == L and b == L exactly (in), then L one step above both (out), then only b below L (out)
    pts = [(0, 0, 0), (2, 0, 0)]
    out.append(_table("length_on_L", pts, pts, T, 0.5, 2.0))
    out.append(_table("length_below_L", pts, pts, T, 0.5, float(np.nextafter(T(2), T(3)))))
    out.append(_table("b_below_L", [(0, 0, 0), (2.25, 0, 0)], [(0, 0, 0), (1.875, 0, 0)], T, 0.5, 2.0))
    # duplicate source points (A = 0) and duplicate target points (B = 0): compatible at L = 0 when the other length is inside thr, never at L > 0
    dup_x = [(1, 1, 1), (1, 1, 1), (1, 1, 1.03125), (4, 1, 1)]
    dup_y = [(2, 2, 2), (2, 2, 2.03125), (2, 2, 2), (5, 2, 2)]
    out.append(_table("duplicates", dup_x, dup_y, T, 0.0625, 0.0))
    out.append(_table("duplicates_min_length", dup_x, dup_y, T, 0.0625, 0.015625))
    # several matches on one target row (idx repeats): B = 0 between them
    sx, sy = [(0, 0, 0), (0.03125, 0, 0), (3, 0, 0), (3, 4, 0)], [(1, 1, 1), (9, 9, 9), (4, 1, 1), (4, 5, 1)]
    out.append(_table("shared_target", sx, sy, T, 0.0625, 0.0, idx=[0, 0, 2, 3]))
    out.append(_table("shared_target_min_length", sx, sy, T, 0.0625, 0.0625, idx=[0, 0, 2, 3]))
    # rows that are not live: a NaN and an inf coordinate, idx = -1
    x = [(0, 0, 0), (np.nan, 0, 0), (3, 4, 0), (1, 1, 1), (6, 8, 0), (2, 2, 2)]
    y = [(0, 0, 0), (1, 0, 0), (3, 4, 0), (np.inf, 1, 1), (6, 8, 0), (2, 2, 2)]
    out.append(_table("not_live", x, y, T, 0.25, 0.0, idx=[0, 1, 2, 3, 4, -1]))
    # all scores tied: an exact copy (every pair compatible, every score 1): the rank is the position
    lat = [(i, (3 * i) % 5, (7 * i) % 4) for i in range(9)]
    out.append(_table("all_tied", lat, lat, T, 0.25))
    # two disjoint cliques of equal size: the second one shifted exactly, its x scaled by 2 against the first: no pair across is compatible
    ca = [(i, (3 * i) % 5, (7 * i) % 4) for i in range(5)]
    cb = [(40 + 2 * i, (5 * i) % 7, i) for i in range(5)]
    xs = [p for pq in zip(ca, cb) for p in pq]                  # interleaved
    ys = [p for pq in zip(ca, [(a + 100, b, c + 3) for a, b, c in cb]) for p in pq]
    out.append(_table("two_cliques", xs, ys, T, 0.25))
    return out


def few_pairs(dtype, P, n=7):
    """a cloud of n matches of which P in {0, 1, 2, 3} are live (the others idx = -1), the live ones an exact copy"""
    x = np.array([(i, (2 * i) % 3, i % 2) for i in range(n)], dtype=dtype)
    idx = np.full(n, -1, dtype=np.int64)
    live = [5, 1, 3][:P]
    idx[live] = live
    return _table("P%d" % P, x, x.copy(), dtype, 0.25, idx=idx)


# ------------------------------------------------------------------ random clouds
def cloud(rng, n, m, P, dtype, rows=None, inlier_ratio=0.3, noise=0.01, clamp=True):
    """One cloud with exactly P live pairs among its first `rows` rows, coordinates of order 10: x uniform in [0, 10]^3, y = C x + r + noise for
    the inliers and uniform for the rest, idx an injection into y where n <= m - 1.  The other rows are not live, each for another reason in
    turn: idx < 0, a NaN in x, an inf in the matched row of y; rows at and past `rows` are padding holding NaN and 1e30 with indices in and
    out of range.  With clamp, one live row names a row of y at or past m (clamped to m - 1).  -> x (n, 3), y (m, 3), idx (n,) int64"""
    rows = n if rows is None else rows
    C, r = rr.rotation(rng), rng.uniform(-0.5, 0.5, 3)
    x = rng.uniform(0.0, 10.0, (n, 3))
    to = rng.permutation(m - 1)[:n] if n <= m - 1 else rng.integers(0, m - 1, n)
    y = rng.uniform(0.0, 10.0, (m, 3))
    good = rng.random(n) < inlier_ratio
    y[to[good]] = x[good] @ C.T + r + noise * rng.standard_normal((int(good.sum()), 3))
    idx = to.astype(np.int64)
    livepos = np.sort(rng.permutation(rows)[:P])
    dead = np.setdiff1d(np.arange(rows), livepos)
    x, y = x.astype(dtype), y.astype(dtype)
    for k, i in enumerate(dead):
        if k % 3 == 0:
            idx[i] = -1 - (k % 5)
        elif k % 3 == 1:
            x[i, k % 2] = np.nan
        elif n <= m - 1:
            y[idx[i], 2] = np.inf
        else:
            idx[i] = -1
    if clamp and P > 8:
        i = livepos[3]
        y[m - 1] = (x[i].astype(np.float64) @ C.T + r).astype(dtype)
        idx[i] = m + 5
    x[rows:] = np.nan
    x[rows + 1::2] = 1e30
    idx[rows:] = rng.integers(-3, m + 9, n - rows)
    if n - rows >= 2:
        idx[rows], idx[rows + 1] = m + 7, -2
    return x, y, idx
