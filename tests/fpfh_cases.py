"""Inputs that the CPU and the GPU tests of the FPFH descriptor share (tests/test_fpfh_host.py, tests/test_gpu_fpfh.py): random clouds with
every kind of dead row and garbage index, the designed clouds, batches of them, and the structured scene of the end-to-end test.
"""
import numpy as np

import fpfh_ref as fr

GARBAGE = (-1, -7, 1 << 40, -(1 << 40), (1 << 31) - 1)


def rotation(axis, angle):
    ax = np.asarray(axis, dtype=np.float64)
    ax = ax / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def index_dtype(idx, dtype):
    """an index array as int32 / int64: values beyond int32 become other out-of-range values"""
    if dtype == np.int64:
        return idx.astype(np.int64)
    return np.where(np.abs(idx) > (1 << 31) - 1, np.sign(idx) * ((1 << 31) - 1), idx).astype(np.int32)


# ------------------------------------------------------------------ random clouds
def random_cloud(seed, m, k, dtype, rows=None, cols=3, planar=False, garbage=True):
    """-> dict points (m, cols), normals (m, 3), idx (m, k) int64, d2 (m, k) the search's own, rows.  The neighbours are the k nearest rows
    (the row itself among them); with garbage: a NaN coordinate, a zero normal, a NaN normal, an inf normal, exact duplicates, slots
    overwritten with -1, -7, huge values and rows at or past `rows`; rows at and past `rows` hold NaN; columns past 2 hold NaN."""
    rng = np.random.default_rng(seed)
    rows = m if rows is None else rows
    P = rng.uniform(-1.0, 1.0, (m, 3))
    if planar:
        P[:, 2] = 0.05 * np.sin(3.0 * P[:, 0]) * np.cos(2.0 * P[:, 1])
    Nn = unit(rng.standard_normal((m, 3)))
    if planar:
        Nn = unit(np.array([0.0, 0.0, 1.0]) + 0.3 * rng.standard_normal((m, 3)))
    P, Nn = P.astype(dtype), Nn.astype(dtype)
    if garbage and rows >= 12:
        P[3, 1] = np.nan
        Nn[5] = 0.0
        Nn[7, 2] = np.nan
        Nn[9, 0] = np.inf
        P[11] = P[10]                                               # an exact duplicate: distance 0
    d2, idx = fr.knn_self(P, k, rows)
    if garbage:
        hit = rng.random((m, k)) < 0.08
        idx[hit] = rng.choice(np.array(GARBAGE + (rows, rows + 1, m + 5), dtype=np.int64), int(hit.sum()))
        if rows >= 4:
            idx[2, -1] = 2                                          # the row itself in the last slot
    P[rows:] = np.nan
    Nn[rows:] = np.nan
    idx[rows:] = rng.integers(-3, m + 3, (m - rows, k))
    pts = np.full((m, cols), np.nan, dtype=dtype)
    pts[:, :3] = P
    return dict(points=pts, normals=Nn, idx=idx, d2=d2.astype(dtype), rows=rows)


# ------------------------------------------------------------------ designed clouds
FRAME = rotation([0.3, -0.5, 0.8], 0.7)         # a frame without zero components


def pair_from_features(theta, alpha, phi, R=FRAME, length=0.5):
    """two points and normals whose pair features are (theta, alpha, phi) with point 0 the source: |phi| >= |n2 . d| is the caller's affair
    -> p (2, 3), n (2, 3)"""
    n1, u = R @ np.array([0.0, 0.0, 1.0]), R @ np.array([1.0, 0.0, 0.0])
    d = phi * n1 + np.sqrt(1.0 - phi * phi) * u
    v = np.cross(u, n1)                                             # = d x n1 normalised; w = n1 x v = u
    n2 = alpha * v + np.sqrt(1.0 - alpha * alpha) * (np.cos(theta) * n1 + np.sin(theta) * u)
    return np.stack((np.zeros(3), length * d)), np.stack((n1, n2))


def unit_centre(t):
    return (t + 0.5) / 11.0 * 2.0 - 1.0


def theta_centre(t):
    return -np.pi + 2.0 * np.pi * (t + 0.5) / 11.0


def bin_centres(dtype):
    """33 pairs far from each other, pair p at the centre of bin p of its feature (the other two features well inside a bin, and chosen so
    that point 0 stays the source) -> the cloud (66 rows, k = 2: the partner, then an empty slot) and channel[p]"""
    specs = [(theta_centre(t), unit_centre(8), unit_centre(10)) for t in range(11)]
    specs += [(theta_centre(8), unit_centre(t), unit_centre(10)) for t in range(11)]
    specs += [(theta_centre(5), unit_centre(8), unit_centre(t)) for t in range(11)]
    P, Nn, idx = [], [], []
    for p, (th, al, ph) in enumerate(specs):
        pp, nn = pair_from_features(th, al, ph)
        P.append(pp + np.array([10.0 * p, 0.0, 0.0]))
        Nn.append(nn)
        idx += [[2 * p + 1, -1], [2 * p, -1]]
    return dict(points=np.concatenate(P).astype(dtype), normals=np.concatenate(Nn).astype(dtype), idx=np.array(idx, dtype=np.int64), rows=66,
                channel=np.arange(33))


def cloud_of(points, normals, idx, dtype, rows=None):
    points = np.asarray(points, dtype=np.float64).astype(dtype)
    return dict(points=points, normals=np.asarray(normals, dtype=np.float64).astype(dtype), idx=np.asarray(idx, dtype=np.int64),
                rows=points.shape[0] if rows is None else rows)


def clamp_pairs(dtype):
    """alpha = +1 and alpha = -1 exactly (the clamp at 11 and the bin 0), from axis-aligned vectors: rows 0-1 and 2-3"""
    P = [[0, 0, 0], [1, 0, 1], [10, 0, 0], [11, 0, 1]]
    Nn = [[0, 0, 1], [0, -1, 0], [0, 0, 1], [0, 1, 0]]
    return cloud_of(P, Nn, [[1], [0], [3], [2]], dtype)


def theta_pi(dtype):
    """theta = pi: n2 = -n1, cos = -1 and sin = +0 or -0.  Pairs over the sign patterns of the zero components of n1 and n2: the reference
    finds both signs of the zero among them (test_fpfh_host.py asserts so).  |a1| = |a2| on every pair: ties."""
    P, Nn, idx = [], [], []
    z = (0.0, -0.0)
    q = 0
    for a in z:
        for b in z:
            for c in z:
                for e in z:
                    P += [[10.0 * q, 0, 0], [10.0 * q + 1, 0, 1]]
                    Nn += [[a, b, 1.0], [c, e, -1.0]]
                    idx += [[2 * q + 1], [2 * q]]
                    q += 1
    return cloud_of(P, Nn, idx, dtype)


def tie(dtype):
    """|a1| = |a2| exactly, on mirrored normals: a swap on the tie would change phi's sign"""
    return cloud_of([[0, 0, 0], [1, 0, 0]], [[0.6, 0.8, 0], [0.6, -0.8, 0]], [[1], [0]], dtype)


def parallel(dtype):
    """d parallel to n1: rows 0 and 1 are near but have no frame; row 1 has a second neighbour, row 2, with one -- so row 0, without a
    pair of its own, still receives row 1's SPFH"""
    pp, nn = pair_from_features(theta_centre(3), unit_centre(7), unit_centre(9), R=np.eye(3))      # (its n1 is (0, 0, 1), row 1's normal)
    P = [[0, 0, 0], [0, 0, 2], np.array([0.0, 0, 2]) + pp[1]]
    Nn = [[0, 0, 1], [0, 0, 1], nn[1]]
    return cloud_of(P, Nn, [[1, -1], [0, 2], [1, -1]], dtype)


def dead_rows(dtype):
    """duplicates, zero / NaN / inf normals, a NaN coordinate, the row itself, garbage indices: row 0 names all of them and row 8, the only
    live neighbour"""
    P = [[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [np.nan, 0, 0], [1, 1, 0], [1, 1, 1], [0.5, 0.2, 0.1], [0.4, 0.1, 0.3]]
    Nn = [[0, 0, 1], [0, 1, 0], [0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0], [0, 0, 1], [0, 0, 1], [1, 0, 0], [0.6, 0, 0.8], [0, 0.6, 0.8]]
    k = 16
    idx = np.full((10, k), -1, dtype=np.int64)
    idx[0, :14] = [0, 1, 2, 3, 4, 5, -1, -7, 10, 11, 1 << 40, -(1 << 40), 8, 0]
    idx[8, :3] = [0, 9, 8]
    idx[9, :2] = [8, 9]
    idx[1, :2] = [0, 8]                                             # (the duplicate: its slot to row 0 is at distance 0)
    idx[6:8] = np.arange(k) % 12                                    # two rows that name every row, the dead ones and 10, 11 >= rows too
    return cloud_of(P, Nn, idx, dtype, rows=10)


def designed(dtype):
    """name -> cloud"""
    return {"bin_centres": bin_centres(dtype), "clamp": clamp_pairs(dtype), "theta_pi": theta_pi(dtype), "tie": tie(dtype),
            "parallel": parallel(dtype), "dead_rows": dead_rows(dtype)}


# ------------------------------------------------------------------ batches
def pad_batch(clouds, m=None, k=None):
    """clouds (dicts) -> points (N, m, c), normals (N, m, 3), idx (N, m, k) int64, rows (N,): pad rows hold NaN and slots of every kind, pad
    slots -1"""
    m = max(c["points"].shape[0] for c in clouds) if m is None else m
    k = max(c["idx"].shape[1] for c in clouds) if k is None else k
    cols, dtype = clouds[0]["points"].shape[1], clouds[0]["points"].dtype
    N = len(clouds)
    P = np.full((N, m, cols), np.nan, dtype=dtype)
    Nn = np.full((N, m, 3), np.nan, dtype=dtype)
    idx = np.full((N, m, k), -1, dtype=np.int64)
    rows = np.zeros(N, dtype=np.int32)
    for b, c in enumerate(clouds):
        mb, kb = c["idx"].shape
        P[b, :mb], Nn[b, :mb], idx[b, :mb, :kb], rows[b] = c["points"], c["normals"], c["idx"], c["rows"]
        idx[b, mb:] = np.arange((m - mb) * k).reshape(m - mb, k) % (m + 2) - 1
    return P, Nn, idx, rows


# ------------------------------------------------------------------ the structured scene
SCENE_SIZE = 10.0
VIEWPOINT = np.array([5.0, 5.0, 25.0])
BOXES = ((2.0, 2.5, 1.6, 1.2, 1.0), (7.0, 2.0, 1.2, 2.0, 1.5), (3.0, 7.0, 2.2, 1.4, 0.8), (7.5, 7.0, 1.5, 1.5, 2.0))      # cx, cy, wx, wy, height


def scene(seed=0, m=1500):
    """A bumpy height field with four boxes over [0, 10]^2, m points at random places -> (m, 3) float64"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, SCENE_SIZE, (m, 2))
    bumps = rng.uniform(0.0, SCENE_SIZE, (80, 2))                  # bumps of the size of a descriptor's support: flat patches all look alike
    amp, sig = rng.uniform(-0.6, 0.6, 80), rng.uniform(0.3, 0.8, 80)
    z = np.zeros(m)
    for (cx, cy), a, s in zip(bumps, amp, sig):
        z += a * np.exp(-((xy[:, 0] - cx) ** 2 + (xy[:, 1] - cy) ** 2) / (2 * s * s))
    for cx, cy, wx, wy, h in BOXES:
        inside = (np.abs(xy[:, 0] - cx) < wx / 2) & (np.abs(xy[:, 1] - cy) < wy / 2)
        z[inside] += h
    return np.concatenate((xy, z[:, None]), axis=1)


def normals_np(points, k, viewpoint):
    """PCA normals over the k nearest rows, facing the viewpoint (numpy; the GPU tests use estimate_normals)"""
    _, idx = fr.knn_self(points, k)
    Q = points[idx]
    Q = Q - Q.mean(axis=1, keepdims=True)
    C = np.einsum("mki,mkj->mij", Q, Q)
    _, vec = np.linalg.eigh(C)
    n = vec[:, :, 0]
    flip = ((viewpoint - points) * n).sum(-1) < 0
    n[flip] = -n[flip]
    return n


E2E_AXIS = (0.2, 0.1, 1.0)      # the end-to-end test turns the scene about a nearly vertical axis, as a vehicle turns: ICP alone is then trapped


def moved_copy(points, seed=0, keep=1.0, angle=1.0, noise=0.0, axis=None):
    """A rigidly moved, row-permuted subset -> dict x (the copy), R, t (x = R p + t), src (the row of `points` every row of x came from).
    axis: the rotation axis, a seeded random one if None"""
    rng = np.random.default_rng(100 + seed)
    m = points.shape[0]
    src = rng.permutation(m)[:int(round(keep * m))]
    R, t = rotation(rng.standard_normal(3) if axis is None else axis, angle), np.array([4.0, -6.0, 3.0])
    x = points[src] @ R.T + t + noise * rng.standard_normal((src.size, 3))
    return dict(x=x, R=R, t=t, src=src)


def nearest_rows(fx, fy):
    """the row of fy nearest to every row of fx in descriptor space (brute force, float64) -> (n,) and the mutual mask"""
    fx, fy = fx.astype(np.float64), fy.astype(np.float64)
    D = (fx * fx).sum(1)[:, None] - 2.0 * fx @ fy.T + (fy * fy).sum(1)[None, :]
    to = D.argmin(axis=1)
    back = D.argmin(axis=0)
    return to, back[to] == np.arange(fx.shape[0])
