"""numpy restatement of dicp_amd/csrc/dicp_iss.h (the ISS keypoints of dicp_amd/iss.py), for the CPU and GPU tests.

Everything is float64 on the exactly converted inputs; numpy rounds every operation on its own, as the header does with one statement per
product.  The functions take keyword switches for WRONG rules, which the tests show the comparison to refuse.
"""
import numpy as np

SWEEPS = 6


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def row_ok(P):
    return np.isfinite(P).all(-1)


def members(P, ok, idx, rows, radius, keep_self=False):
    """the member slots of every row -> (mem (m, k) bool, q (m, k, 3) = p_j - p_i, jc (m, k) the clamped rows)"""
    m = P.shape[0]
    j = np.asarray(idx).astype(np.int64)
    live = (j >= 0) & (j < rows)
    if not keep_self:
        live &= j != np.arange(m)[:, None]
    jc = np.where(live, j, 0)
    with np.errstate(all="ignore"):
        q = P[jc] - P[:, None, :]
        x = q[..., 0] * q[..., 0]
        y = q[..., 1] * q[..., 1]
        z = q[..., 2] * q[..., 2]
        r2 = (x + y) + z
        mem = live & ok[:, None] & ok[jc]
        if radius is not None:
            mem &= r2 <= float(radius) * float(radius)
    return mem, q, jc


def covariance(mem, q, count):
    """the six entries (xx, xy, xz, yy, yz, zz) over the row itself (q = 0) and the member slots, in that order -> list of six (m,)"""
    m, k = mem.shape
    with np.errstate(all="ignore"):
        n = count.astype(np.float64)
        s = np.zeros((m, 3))
        for sl in range(k):
            s = np.where(mem[:, sl, None], s + q[:, sl], s)
        mu = s / n[:, None]
        a = [np.zeros(m) for _ in range(6)]
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        d = 0.0 - mu
        for e, (u, v) in enumerate(pairs):
            a[e] = a[e] + d[:, u] * d[:, v]
        for sl in range(k):
            d = q[:, sl] - mu
            for e, (u, v) in enumerate(pairs):
                a[e] = np.where(mem[:, sl], a[e] + d[:, u] * d[:, v], a[e])
        return [x / n for x in a]


def rotate(app, aqq, apq, arp, arq):
    with np.errstate(all="ignore"):
        on = apq != 0.0
        diff = aqq - app
        two = 2.0 * apq
        zeta = diff / two
        zz = zeta * zeta
        h = 1.0 + zz
        den = np.abs(zeta) + np.sqrt(h)
        t = np.where(zeta < 0.0, -1.0, 1.0) / den
        tt = t * t
        g = 1.0 + tt
        c = 1.0 / np.sqrt(g)
        s = c * t
        u = t * apq
        cp, sq, sp, cq = c * arp, s * arq, s * arp, c * arq
        return (np.where(on, app - u, app), np.where(on, aqq + u, aqq), np.where(on, 0.0, apq), np.where(on, cp - sq, arp),
                np.where(on, sp + cq, arq))


def exchange(lo, hi):
    sw = lo > hi
    return np.where(sw, hi, lo), np.where(sw, lo, hi)


def eigenvalues(a, sweeps=SWEEPS, return_needed=False, return_worked=False):
    """a: the six entries (xx, xy, xz, yy, yz, zz), each (n,) float64 -> (n, 3) ascending[, the sweeps after which every off-diagonal was
    exactly 0, sweeps + 1 where they never were][, the six entries as the sweeps left them (n, 6)]"""
    a = [np.array(x, dtype=np.float64) for x in a]
    needed = np.full(a[0].shape, sweeps + 1, dtype=np.int64)
    needed[(a[1] == 0.0) & (a[2] == 0.0) & (a[4] == 0.0)] = 0
    for it in range(sweeps):
        a[0], a[3], a[1], a[2], a[4] = rotate(a[0], a[3], a[1], a[2], a[4])
        a[0], a[5], a[2], a[1], a[4] = rotate(a[0], a[5], a[2], a[1], a[4])
        a[3], a[5], a[4], a[1], a[2] = rotate(a[3], a[5], a[4], a[1], a[2])
        done = (a[1] == 0.0) & (a[2] == 0.0) & (a[4] == 0.0)
        needed = np.where(done & (needed > it + 1), it + 1, needed)
    l0, l1, l2 = a[0], a[3], a[5]
    l0, l1 = exchange(l0, l1)
    l1, l2 = exchange(l1, l2)
    l0, l1 = exchange(l0, l1)
    lam = np.stack((l0, l1, l2), axis=-1)
    out = (lam,) + ((needed,) if return_needed else ()) + ((np.stack(a, axis=-1),) if return_worked else ())
    return out if len(out) > 1 else lam


def saliency_rule(lam, count, gamma21, gamma32, min_neighbors, gamma_le=False):
    with np.errstate(all="ignore"):
        b21 = gamma21 * lam[..., 2]
        b32 = gamma32 * lam[..., 1]
        if gamma_le:
            good = (count >= min_neighbors) & (lam[..., 1] <= b21) & (0.0 < lam[..., 0]) & (lam[..., 0] <= b32)
        else:
            good = (count >= min_neighbors) & (lam[..., 1] < b21) & (0.0 < lam[..., 0]) & (lam[..., 0] < b32)
    return np.where(good, lam[..., 0], 0.0)


def _cloud(points, rows):
    m = points.shape[0]
    rows = m if rows is None else int(min(max(rows, 0), m))
    P = np.asarray(points)[:, :3].astype(np.float64)
    ok = row_ok(P)
    ok[rows:] = False
    return P, ok, rows


def iss_ref(points, idx, rows=None, radius=None, gamma21=0.975, gamma32=0.975, min_neighbors=5, sweeps=SWEEPS, gamma_le=False, self_twice=False):
    """One cloud: points (m, >= 3), idx (m, k) -> dict eig (m, 3) and sal (m,) in the points' dtype, sal64 (m,) the double saliency, count
    (m,) int32.

    Wrong rules: sweeps other than 6; gamma_le asks <= of the two gamma tests; self_twice does not skip a slot that names the row itself."""
    P, ok, rows = _cloud(points, rows)
    mem, q, _ = members(P, ok, idx, rows, radius, keep_self=self_twice)
    count = np.where(ok, 1 + mem.sum(axis=1), 0)
    lam = eigenvalues(covariance(mem, q, np.where(ok, count, 1)), sweeps)
    lam = np.where(ok[:, None], lam, 0.0)
    sal = np.where(ok, saliency_rule(lam, count, gamma21, gamma32, min_neighbors, gamma_le), 0.0)
    dt = np.asarray(points).dtype
    return dict(eig=lam.astype(dt), sal=sal.astype(dt), sal64=sal, count=count.astype(np.int32))


def maxima_ref(points, idx, sal64, rows=None, radius=None, min_neighbors=5, tie_both=False, no_radius=False):
    """One cloud: the keypoint mask (m,) bool from the double saliencies.  Wrong rules: tie_both keeps both sides of an exact tie;
    no_radius drops the radius cut."""
    P, ok, rows = _cloud(points, rows)
    mem, _, jc = members(P, ok, idx, rows, None if no_radius else radius)
    count = 1 + mem.sum(axis=1)
    si, sj = sal64[:, None], sal64[jc]
    beats = sj > si
    if not tie_both:
        beats |= (sj == si) & (jc < np.arange(P.shape[0])[:, None])
    return ok & (sal64 > 0.0) & (count >= min_neighbors) & ~(mem & beats).any(axis=1)


def keypoints_ref(points, idx, rows=None, salient_radius=None, non_max_radius=None, gamma21=0.975, gamma32=0.975, min_neighbors=5, nms_idx=None,
                  sweeps=SWEEPS, gamma_le=False, self_twice=False, tie_both=False, no_radius=False):
    """One cloud -> iss_ref's dict with mask (m,) bool added"""
    out = iss_ref(points, idx, rows, salient_radius, gamma21, gamma32, min_neighbors, sweeps=sweeps, gamma_le=gamma_le, self_twice=self_twice)
    out["mask"] = maxima_ref(points, idx if nms_idx is None else nms_idx, out["sal64"], rows, non_max_radius, min_neighbors, tie_both=tie_both,
                             no_radius=no_radius)
    return out


def keypoints_ref_batch(points, idx, rows=None, nms_idx=None, **kw):
    """(N, m, c), (N, m, k), rows a sequence or None -> dict of stacked eig (N, m, 3), sal, sal64, count, mask (N, m)"""
    outs = [keypoints_ref(points[b], idx[b], None if rows is None else rows[b], nms_idx=None if nms_idx is None else nms_idx[b], **kw)
            for b in range(points.shape[0])]
    return {key: np.stack([o[key] for o in outs]) for key in outs[0]}


def same(got, want, keys=("eig", "sal", "count", "mask")):
    """eigenvalues, saliency and counts bit for bit, the mask exactly"""
    return all(same_bits(got[key], want[key]) for key in keys)


def knn_self(points, k, rows=None):
    """brute force: the k nearest rows of every row of one cloud (itself included) in (d2, index) order -> d2 (m, k) float64, idx (m, k)
    int64 with inf / -1 in empty slots; rows with a non-finite coordinate find nothing and are found by nobody"""
    P = np.asarray(points)[:, :3].astype(np.float64)
    m = P.shape[0]
    rows = m if rows is None else rows
    with np.errstate(all="ignore"):
        D = ((P[:, None, :] - P[None, :, :]) ** 2).sum(-1)
    D[:, rows:] = np.inf
    D[rows:, :] = np.inf
    D[~np.isfinite(D)] = np.inf
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    d2 = np.take_along_axis(D, order, axis=1)
    idx = np.where(np.isfinite(d2), order, -1).astype(np.int64)
    if idx.shape[1] < k:
        idx = np.concatenate((idx, np.full((m, k - idx.shape[1]), -1, np.int64)), axis=1)
        d2 = np.concatenate((d2, np.full((m, k - d2.shape[1]), np.inf)), axis=1)
    return d2, idx
