"""numpy restatement of dicp_amd.fps.sample_farthest_points for one cloud: the definition of its docstring, vectorised per step, in the
points' own dtype (so every rounding is the kernel's).  tie_high / repick are deliberately WRONG variants (ties to the highest index;
picked rows stay in play) that the tests use to show that their inputs tell the rule from its neighbours."""
import numpy as np


def fps_ref(p, k, rows=None, start=0, tie_high=False, repick=False):
    """p (n, c) float32 / float64 -> (idx (k,) int64, dist (k,) p.dtype, k_eff); slots at or past k_eff hold -1 / +inf"""
    n = p.shape[0] if rows is None else int(rows)
    xyz = p[:n, :3]
    idx, dist = np.full(k, -1, np.int64), np.full(k, np.inf, p.dtype)
    cand = np.isfinite(xyz).all(1)
    if not cand.any():
        return idx, dist, 0
    rank = (np.arange(n) - int(start)) % n
    pick = int(np.argmin(np.where(cand, rank, n)))
    D = np.where(cand, np.inf, -1).astype(p.dtype)
    for t in range(k):
        if t:
            if not (D >= 0).any():
                return idx, dist, t
            pick = int(n - 1 - np.argmax(D[::-1])) if tie_high else int(np.argmax(D))      # (argmax: the first of the equal maxima)
            dist[t] = D[pick]
        idx[t] = pick
        with np.errstate(all="ignore"):
            dx, dy, dz = xyz[pick, 0] - xyz[:, 0], xyz[pick, 1] - xyz[:, 1], xyz[pick, 2] - xyz[:, 2]
            d = (dx * dx + dy * dy) + dz * dz
        D = np.where((D >= 0) & (d < D), d, D)
        if not repick:
            D[pick] = -1
    return idx, dist, k
