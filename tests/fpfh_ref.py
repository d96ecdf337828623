"""numpy restatement of dicp_amd/csrc/dicp_fpfh.h (the FPFH descriptor of dicp_amd/fpfh.py), for the CPU and GPU tests.

Everything is float64 on the exactly converted inputs; numpy rounds every operation on its own, as the header does with one statement per
product.  fpfh_ref takes keyword switches for WRONG rules, which the tests show the comparison to refuse.
"""
import numpy as np

BINS, CH = 11, 33
# (cos, sin) of the bin edges beta_t = -pi + 2 pi t / 11, t = 1 .. 10: the literals of fpfh_bin_theta
EDGES = (
    (-0.8412535328311811, -0.5406408174555978),
    (-0.4154150130018863, -0.9096319953545184),
    (0.14231483827328512, -0.9898214418809327),
    (0.6548607339452851, -0.7557495743542583),
    (0.9594929736144975, -0.2817325568414295),
    (0.9594929736144975, 0.2817325568414295),
    (0.6548607339452851, 0.7557495743542583),
    (0.14231483827328512, 0.9898214418809327),
    (-0.41541501300188616, 0.9096319953545186),
    (-0.8412535328311813, 0.5406408174555974),
)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def dot(a, b):
    x = a[..., 0] * b[..., 0]
    y = a[..., 1] * b[..., 1]
    z = a[..., 2] * b[..., 2]
    return (x + y) + z


def cross(a, b):
    a, b = np.broadcast_arrays(a, b)
    c0 = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
    c1 = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
    c2 = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    return np.stack((c0, c1, c2), axis=-1)


def bin_unit(a):
    x = 11.0 * ((a + 1.0) * 0.5)
    out = np.zeros(x.shape, dtype=np.int64)
    mid = (x >= 1.0) & (x < 10.0)
    out[mid] = x[mid].astype(np.int64)
    out[x >= 10.0] = 10
    return out


def bin_theta(c, s, strict_edge=False):
    out = np.zeros(np.shape(c), dtype=np.int64)
    for cb, sb in EDGES:
        cr = cb * s - sb * c
        up = (s > 0.0) if strict_edge else (s >= 0.0)
        out += ((up | (cr >= 0.0)) if sb < 0.0 else ((s >= 0.0) & (cr >= 0.0))).astype(np.int64)
    return out


def bin_theta_atan2(c, s):
    """the libm form the half-plane rule stands for -> (bin, the distance to the nearest edge in bins)"""
    x = 11.0 * (np.arctan2(s, c) + np.pi) / (2.0 * np.pi)
    return np.clip(np.floor(x), 0, 10).astype(np.int64), np.abs(x - np.round(x))


def pair_features(pi, ni, pj, nj, tie_swap=False):
    """float64 arrays (..., 3) -> dict r2, cos, sin, alpha, phi, frame (no radius, no OK test)"""
    with np.errstate(all="ignore"):
        d = pj - pi
        r2 = dot(d, d)
        r = np.sqrt(r2)
        a1 = dot(ni, d) / r
        a2 = dot(nj, d) / r
        swap = (np.abs(a1) <= np.abs(a2)) if tie_swap else (np.abs(a1) < np.abs(a2))
        n1 = np.where(swap[..., None], nj, ni)
        n2 = np.where(swap[..., None], ni, nj)
        d = np.where(swap[..., None], -d, d)
        phi = np.where(swap, -a2, a1)
        v = cross(d, n1)
        q = dot(v, v)
        v = v / np.sqrt(q)[..., None]
        w = cross(n1, v)
        return dict(r2=r2, cos=dot(n1, n2), sin=dot(w, n2), alpha=dot(v, n2), phi=phi, frame=q > 0.0)


def row_ok(P, Nn):
    return np.isfinite(P).all(-1) & np.isfinite(Nn).all(-1) & (Nn != 0.0).any(-1)


def fpfh_ref(points, normals, idx, rows=None, radius=None, tie_swap=False, strict_edge=False, keep_self=False, search_d2=None, norm_k=False):
    """One cloud: points (m, >= 3), normals (m, 3), idx (m, k) -> (out (m, 33) in the points' dtype, cnt (m, 33) uint8).

    Wrong rules: tie_swap swaps on |a1| = |a2| too; strict_edge asks sin > 0 of a lower-half-plane edge; keep_self leaves the row itself
    (and any slot at distance 0) among its neighbours; search_d2 (m, k) weights by the search's d2; norm_k divides the counts by k."""
    m, k = idx.shape
    rows = m if rows is None else int(min(max(rows, 0), m))
    P = np.asarray(points)[:, :3].astype(np.float64)
    Nn = np.asarray(normals).astype(np.float64)
    ok = row_ok(P, Nn)
    ok[rows:] = False
    j = np.asarray(idx).astype(np.int64)
    live = (j >= 0) & (j < rows)
    if not keep_self:
        live &= j != np.arange(m)[:, None]
    jc = np.where(live, j, 0)
    f = pair_features(P[:, None, :], Nn[:, None, :], P[jc], Nn[jc], tie_swap=tie_swap)
    with np.errstate(all="ignore"):
        r2 = f["r2"]
        near = live & ok[:, None] & ok[jc]
        if not keep_self:
            near &= r2 > 0.0
        if radius is not None:
            near &= r2 <= float(radius) * float(radius)
        pair = near & f["frame"]
        ii = np.broadcast_to(np.arange(m)[:, None], (m, k))
        cnt = np.zeros((m, CH), dtype=np.int64)
        for b in (bin_theta(f["cos"], f["sin"], strict_edge), BINS + bin_unit(f["alpha"]), 2 * BINS + bin_unit(f["phi"])):
            np.add.at(cnt, (ii[pair], b[pair]), 1)
        c = pair.sum(axis=1)
        den = np.where(c > 0, k if norm_k else c, 1).astype(np.float64)
        s = np.where((c > 0)[:, None], (100.0 * cnt.astype(np.float64)) / den[:, None], 0.0)
        wsrc = r2 if search_d2 is None else np.asarray(search_d2).astype(np.float64)
        acc = np.zeros((m, CH))
        for sl in range(k):
            wj = 1.0 / wsrc[:, sl]
            t = wj[:, None] * s[jc[:, sl]]
            acc = np.where(near[:, sl, None], acc + t, acc)
        out = np.zeros((m, CH))
        for g in range(3):
            S = np.zeros(m)
            for a in range(BINS):
                S = S + acc[:, g * BINS + a]
            fac = 100.0 / S
            u = np.where((S != 0.0)[:, None], acc[:, g * BINS:(g + 1) * BINS] * fac[:, None], 0.0)
            out[:, g * BINS:(g + 1) * BINS] = u + s[:, g * BINS:(g + 1) * BINS]
        return out.astype(np.asarray(points).dtype), cnt.astype(np.uint8)


def fpfh_ref_batch(points, normals, idx, rows=None, radius=None, **kw):
    """(N, m, c), (N, m, 3), (N, m, k), rows a sequence or None -> (out (N, m, 33), cnt (N, m, 33) uint8)"""
    outs = [fpfh_ref(points[b], normals[b], idx[b], None if rows is None else rows[b], radius, **kw) for b in range(points.shape[0])]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


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
