"""The definition of dicp_amd.match.correspondence_compatibility / prune_correspondences in numpy, for one cloud (rules 1-5 of the
docstrings).

Everything is one numpy operation per rounding in the points' dtype T.  The two fma chains use the correctly rounded fma of
tests/match_ref.py for float32 and, for float64, ransac_ref.fma64_fast -- the vectorised emulation that tests/test_ransac_host.py and
tests/test_compat_host.py hold to match_ref.fma64's exact rational arithmetic (the exact one takes a Fraction per element: too slow for
P^2 pairs).  numpy's sqrt and / are the correctly rounded ones of T.  The sequential sum of rule 4 is a loop over q, vectorised over p.

`wrong=` makes the deliberately wrong restatements the tests show the comparisons to refuse.  A plain module (no fixtures): the tests put
this directory on sys.path and import it.
"""
import numpy as np

import ransac_ref as rr

WRONG = ("no_self", "descending", "pairwise", "strict_less", "squared", "sum_norm", "tie_high")


def len2(pts):
    """pts (P, 3) T -> (P, P) T: A[p, q], the fma chain over t_a = pts[p, a] - pts[q, a] from +0"""
    T = pts.dtype.type
    s = np.zeros((pts.shape[0], pts.shape[0]), dtype=pts.dtype)
    with np.errstate(all="ignore"):
        for a in range(3):
            t = (pts[:, None, a] - pts[None, :, a]).astype(T)
            s = rr.fma_t(t, t, s, T).astype(T)
    return s


def relation(pairs, threshold, min_length=0.0, wrong=None):
    """pairs (P, 6) T -> dict A, B, a, b, e (P, P) T and rel (P, P) bool by rule 2, evaluated for every (p, q), the diagonal included"""
    T = pairs.dtype.type
    thr, L = T(threshold), T(min_length)
    A, B = len2(np.ascontiguousarray(pairs[:, :3])), len2(np.ascontiguousarray(pairs[:, 3:]))
    with np.errstate(all="ignore"):
        a, b = np.sqrt(A).astype(T), np.sqrt(B).astype(T)
        e = (a - b).astype(T)
        if wrong == "squared":
            e2 = (A - B).astype(T)
            rel = (e2 <= thr) & (e2 >= -thr)
        elif wrong == "strict_less":
            rel = (e < thr) & (e > -thr)
        else:
            rel = (e <= thr) & (e >= -thr)
        rel = rel & (a >= L) & (b >= L)
    return dict(A=A, B=B, a=a, b=b, e=e, rel=rel)


def degree_of(rel):
    """(P, P) bool -> (P,) int32: the compatible q != p"""
    return (rel & ~np.eye(rel.shape[0], dtype=bool)).sum(axis=1).astype(np.int32)


def _tree(terms):
    """pairwise sum of the columns of terms (P, Q) in T"""
    T = terms.dtype.type
    while terms.shape[1] > 1:
        if terms.shape[1] % 2:
            terms = np.concatenate((terms, np.zeros((terms.shape[0], 1), dtype=terms.dtype)), axis=1)
        terms = (terms[:, 0::2] + terms[:, 1::2]).astype(T)
    return terms[:, 0]


def power(rel, iterations, dtype, wrong=None):
    """rule 4 -> (ws, vs): the w and the v of every iteration, lists of (P,) T; vs[-1] is the score (ones for iterations = 0)"""
    T = np.dtype(dtype).type
    P = rel.shape[0]
    M = rel.copy()
    M[np.arange(P), np.arange(P)] = wrong != "no_self"
    v = np.ones(P, dtype=T)
    ws, vs = [], []
    zero = T(0)
    for _ in range(int(iterations)):
        if wrong == "pairwise":
            w = _tree(np.where(M, v[None, :], zero).astype(T)) if P else np.zeros(0, dtype=T)
        else:
            w = np.zeros(P, dtype=T)
            for q in (range(P - 1, -1, -1) if wrong == "descending" else range(P)):
                w = (w + np.where(M[:, q], v[q], zero)).astype(T)
        if P:
            with np.errstate(all="ignore"):
                den = w.sum(dtype=T) if wrong == "sum_norm" else w.max()
                v = (w / den).astype(T)
        ws.append(w)
        vs.append(v)
    return ws, vs


def ranks(score, wrong=None):
    """rule 5: (P,) T -> (P,) int32"""
    q = np.arange(score.shape[0])
    tie = (q[None, :] > q[:, None]) if wrong == "tie_high" else (q[None, :] < q[:, None])
    before = (score[None, :] > score[:, None]) | ((score[None, :] == score[:, None]) & tie)
    return before.sum(axis=1).astype(np.int32)


def compat_ref(x, y, idx, threshold, iterations=10, min_length=0.0, x_rows=None, keep=None, wrong=None):
    """rules 1-5 for one cloud -> dict: rows (P,), pairs (P, 6), P, rel (P, P), degree_packed, score_packed, ws, vs, score (n,) T and degree
    (n,) int32 in the original row order; with keep also rank_packed (P,), kept (n,) bool and idx_kept (n,) in idx's dtype"""
    dt = x.dtype
    n = x.shape[0]
    rows, pairs = rr.packed(x, y, idx, x_rows)
    P = rows.size
    rel = relation(pairs, threshold, min_length, wrong)["rel"]
    deg = degree_of(rel)
    ws, vs = power(rel, iterations, dt, wrong)
    sp = vs[-1] if vs else np.ones(P, dtype=dt)
    score, degree = np.zeros(n, dtype=dt), np.zeros(n, dtype=np.int32)
    score[rows], degree[rows] = sp, deg
    out = dict(rows=rows, pairs=pairs, P=P, rel=rel, degree_packed=deg, score_packed=sp, ws=ws, vs=vs, score=score, degree=degree)
    if keep is not None:
        rk = ranks(sp, wrong)
        kept = np.zeros(n, dtype=bool)
        kept[rows[rk < keep]] = True
        out.update(rank_packed=rk, kept=kept, idx_kept=np.where(kept, idx, -1).astype(idx.dtype))
    return out


# ------------------------------------------------------------------ the float64 check of the decisions
def relation64(pairs, threshold):
    """the relation | |x_p - x_q| - |y_p - y_q| | <= tau in float64 from the exactly converted inputs -> (rel (P, P) bool, margin (P, P):
    | |e64| - tau |, bound (P, P): 4 u (a + b) + u |e| for the dtype of pairs)"""
    u = 2.0 ** -24 if pairs.dtype == np.float32 else 2.0 ** -53
    p = pairs.astype(np.float64)
    a = np.sqrt(((p[:, None, :3] - p[None, :, :3]) ** 2).sum(-1))
    b = np.sqrt(((p[:, None, 3:] - p[None, :, 3:]) ** 2).sum(-1))
    e = a - b
    return np.abs(e) <= float(threshold), np.abs(np.abs(e) - float(threshold)), 4 * u * (a + b) + u * np.abs(e)


def rotation_angle(C, C_true):
    """the angle of C C_true^T in radians from atan2(|axial part|, (trace - 1) / 2): unlike the arccos of the trace alone it resolves
    angles far below sqrt(u), which float32 poses a few 1e-4 rad from the truth need"""
    R = np.asarray(C, dtype=np.float64).reshape(3, 3) @ np.asarray(C_true, dtype=np.float64).reshape(3, 3).T
    ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0
    return float(np.arctan2(np.linalg.norm(ax), (np.trace(R) - 1.0) / 2.0))


# ------------------------------------------------------------------ inputs the CPU and the GPU tests share
def recovery_case(seed, n=600, inliers=60, noise=0.01, dtype=np.float32):
    """n matches in a 10-unit cube: x uniform in [0, 10]^3; `inliers` of them (shuffled) have y = C x + r + noise, the rest a uniformly
    random target in the cube; idx a permutation -> dict x, y, idx, truth (n,) bool, C (3, 3), r (3,)"""
    rng = np.random.default_rng(2000 + seed)
    C, r = rr.rotation(rng), rng.uniform(-0.5, 0.5, 3)
    x = rng.uniform(0, 10, (n, 3))
    truth = np.zeros(n, dtype=bool)
    truth[rng.permutation(n)[:inliers]] = True
    yi = x @ C.T + r + noise * rng.standard_normal((n, 3))
    yi[~truth] = rng.uniform(0, 10, (int((~truth).sum()), 3))
    perm = rng.permutation(n)
    y = np.empty_like(yi)
    y[perm] = yi
    return dict(x=x.astype(dtype), y=y.astype(dtype), idx=perm.astype(np.int64), truth=truth, C=C, r=r)
