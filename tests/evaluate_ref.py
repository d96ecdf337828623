"""numpy restatement of dicp_amd.evaluate (rules 1-9 of evaluate_registration's docstring) for one pair of clouds and H poses.

The fma chain of the query is ransac_ref.fma_t's correctly rounded fma; r2 and the brute-force match are ball_ref's; the tile tree is
written out level by level.  `wrong=` makes the deliberately wrong restatements the tests show their comparison to refuse:
"ascending" sums every term in ascending row order, "unfused" rounds the products of the query on their own, "tie_high" lets the higher
index win a tie in d2, "strict" compares d2 < r2.

A plain module (no fixtures): the tests put this directory on sys.path and import it."""
import numpy as np

import ball_ref as br
import ransac_ref as rr

TILE, TERMS, H_MAX = 256, 10, 65536
S_E, S_T, S_XX, S_YY, S_ZZ, S_XY, S_XZ, S_YZ = 0, 1, 4, 5, 6, 7, 8, 9


def transform(T, x, wrong=None):
    """rule 2: T (4, 4), x (n, >= 3) of one dtype -> q (n, 3) in that dtype"""
    dt = x.dtype.type
    T = np.asarray(T, dtype=x.dtype)
    q = np.empty((x.shape[0], 3), dtype=x.dtype)
    with np.errstate(all="ignore"):
        for a in range(3):
            v = np.broadcast_to(T[a, 3], (x.shape[0],)).astype(dt)
            for k in range(3):
                if wrong == "unfused":
                    v = (v + (T[a, k] * x[:, k]).astype(dt)).astype(dt)
                else:
                    v = rr.fma_t(np.broadcast_to(T[a, k], (x.shape[0],)).astype(dt), x[:, k], v, dt).astype(dt)
            q[:, a] = v
    return q


def match(q, y, max_distance, x_rows=None, y_rows=None, wrong=None):
    """rule 3 -> idx (n,) int64, d2 (n,) in the dtype: ball_ref at k = 1 (rows of q at or past x_rows, or not finite, have no match)"""
    if wrong == "tie_high":
        n = q.shape[0]
        nb = n if x_rows is None else int(x_rows)
        mb = y.shape[0] if y_rows is None else int(y_rows)
        idx, d2 = np.full(n, -1, np.int64), np.full(n, np.inf, q.dtype)
        if nb and mb:
            D = br.d2_matrix(q[:nb, :3], y[:mb, :3])
            with np.errstate(invalid="ignore"):
                cand = np.isfinite(D) & (D <= br.r2_of(max_distance, q.dtype)) & np.isfinite(q[:nb, :3]).all(1)[:, None]
            for i in np.flatnonzero(cand.any(1)):
                j = np.flatnonzero(cand[i])
                best = j[D[i, j] == D[i, j].min()].max()
                idx[i], d2[i] = best, D[i, best]
        return idx, d2
    d2, idx, _ = br.ball_ref(q, y, max_distance, 1, x_rows=x_rows, y_rows=y_rows, strict=wrong == "strict")
    return idx[:, 0], d2[:, 0]


def terms(idx, d2, y):
    """rule 5 -> (n, 10) float64"""
    n = idx.shape[0]
    v = np.zeros((n, TERMS), dtype=np.float64)
    hit = idx >= 0
    t = y[idx[hit], :3].astype(np.float64)
    v[hit, S_E] = d2[hit].astype(np.float64)
    v[hit, S_T:S_T + 3] = t
    with np.errstate(over="ignore", under="ignore"):
        v[hit, S_XX], v[hit, S_YY], v[hit, S_ZZ] = t[:, 0] * t[:, 0], t[:, 1] * t[:, 1], t[:, 2] * t[:, 2]
        v[hit, S_XY], v[hit, S_XZ], v[hit, S_YZ] = t[:, 0] * t[:, 1], t[:, 0] * t[:, 2], t[:, 1] * t[:, 2]
    return v


def tile_tree(v):
    """rule 6 within a tile: v (256, k) float64 -> (k,)"""
    v = v.copy()
    assert v.shape[0] == TILE
    off = 1
    while off < TILE:
        lo = np.arange(0, TILE, 2 * off)
        v[lo] = v[lo] + v[lo + off]
        off *= 2
    return v[0]


def sums_of(v, wrong=None):
    """rule 6: v (n, k) float64 in row order -> (k,) float64"""
    n, k = v.shape
    total = np.zeros(k, dtype=np.float64)
    if wrong == "ascending":
        for i in range(n):
            total = total + v[i]
        return total
    for c in range((n + TILE - 1) // TILE):
        tile = np.zeros((TILE, k), dtype=np.float64)
        rows = v[c * TILE:(c + 1) * TILE]
        tile[:rows.shape[0]] = rows
        total = total + tile_tree(tile)
    return total


def assemble(sums, count):
    """rule 8: (10,) sums and the count -> (6, 6) float64"""
    S = sums
    L = np.zeros((6, 6), dtype=np.float64)
    L[0, 0], L[1, 1], L[2, 2] = S[S_YY] + S[S_ZZ], S[S_XX] + S[S_ZZ], S[S_XX] + S[S_YY]
    L[0, 1] = L[1, 0] = -S[S_XY]
    L[0, 2] = L[2, 0] = -S[S_XZ]
    L[1, 2] = L[2, 1] = -S[S_YZ]
    sx, sy, sz = S[S_T], S[S_T + 1], S[S_T + 2]
    L[0:3, 3:6] = [[0.0, -sz, sy], [sz, 0.0, -sx], [-sy, sx, 0.0]]
    L[3:6, 0:3] = L[0:3, 3:6].T
    L[3, 3] = L[4, 4] = L[5, 5] = float(count)
    return L


def evaluate_ref(x, y, T, max_distance, x_rows=None, y_rows=None, wrong=None):
    """x (n, c), y (m, c), T (H, 4, 4) of one dtype -> dict: q (H, n, 3), idx (H, n) int64, d2 (H, n), counts (H,) int32, sums (H, 10),
    fitness (H,), rmse (H,) float64, info (H, 6, 6)"""
    T = np.asarray(T, dtype=x.dtype).reshape(-1, 4, 4)
    H, n = T.shape[0], x.shape[0]
    nb = n if x_rows is None else int(x_rows)
    out = dict(q=np.empty((H, n, 3), x.dtype), idx=np.empty((H, n), np.int64), d2=np.empty((H, n), x.dtype), counts=np.zeros(H, np.int32),
               sums=np.zeros((H, TERMS)), fitness=np.zeros(H), rmse=np.zeros(H), info=np.zeros((H, 6, 6)))
    for h in range(H):
        q = transform(T[h], x, wrong)
        idx, d2 = match(q, y, max_distance, x_rows, y_rows, wrong)
        s = sums_of(terms(idx, d2, y), wrong)
        count = int((idx >= 0).sum())
        out["q"][h], out["idx"][h], out["d2"][h], out["counts"][h], out["sums"][h] = q, idx, d2, count, s
        out["fitness"][h] = np.float64(count) / np.float64(nb) if nb > 0 else 0.0
        out["rmse"][h] = np.sqrt(s[S_E] / np.float64(count)) if count > 0 else 0.0
        out["info"][h] = assemble(s, count)
    return out


def best_pose_ref(counts, rmse):
    """rule 9 for one cloud: counts, rmse (H,) -> h"""
    best = 0
    for h in range(1, len(counts)):
        if counts[h] > counts[best] or (counts[h] == counts[best] and rmse[h] < rmse[best]):
            best = h
    return best


def info_plain(y, idx):
    """the independent accumulation of rule 8: the G rows of every matched target point in plain ascending order, float64
    -> (L (6, 6), A (6, 6) the sums of the |terms| of every entry)"""
    L, A = np.zeros((6, 6)), np.zeros((6, 6))
    for j in idx[idx >= 0]:
        tx, ty, tz = (float(v) for v in y[j, :3])
        G = np.array([[0.0, tz, -ty, 1.0, 0.0, 0.0], [-tz, 0.0, tx, 0.0, 1.0, 0.0], [ty, -tx, 0.0, 0.0, 0.0, 1.0]])
        for r in range(3):
            P = np.outer(G[r], G[r])
            L = L + P
            A = A + np.abs(P)
    return L, A
