"""Inputs that the CPU and the GPU tests of the ISS keypoints share (tests/test_iss_host.py, tests/test_gpu_iss.py): random clouds with every
kind of dead row and garbage index, the designed clouds, batches of them, the covariance families of the accuracy test and the cube-corner
scene.
"""
import numpy as np

import iss_ref as ir

GARBAGE = (-1, -7, 1 << 40, -(1 << 40), (1 << 31) - 1)


def index_dtype(idx, dtype):
    """an index array as int32 / int64: values beyond int32 become other out-of-range values"""
    if dtype == np.int64:
        return idx.astype(np.int64)
    return np.where(np.abs(idx) > (1 << 31) - 1, np.sign(idx) * ((1 << 31) - 1), idx).astype(np.int32)


# ------------------------------------------------------------------ random clouds
def random_cloud(seed, m, k, dtype, rows=None, cols=3, planar=False, garbage=True):
    """-> dict points (m, cols), idx (m, k) int64, d2 (m, k) the search's own, rows.  The neighbours are the k nearest rows (the row itself
    among them); with garbage: a NaN and an inf coordinate, exact duplicates, slots overwritten with -1, -7, huge values and rows at or past
    `rows`; rows at and past `rows` hold NaN and slots of every kind; columns past 2 hold NaN."""
    rng = np.random.default_rng(seed)
    rows = m if rows is None else rows
    P = rng.uniform(-1.0, 1.0, (m, 3)) * np.array([1.0, 0.7, 0.45])            # (anisotropic: separated eigenvalues, salient rows)
    if planar:
        P[:, 2] = 0.05 * np.sin(3.0 * P[:, 0]) * np.cos(2.0 * P[:, 1])
    P = P.astype(dtype)
    if garbage and rows >= 12:
        P[3, 1] = np.nan
        P[9, 0] = np.inf
        P[11] = P[10]                                               # an exact duplicate: distance 0
    d2, idx = ir.knn_self(P, k, rows)
    if garbage:
        hit = rng.random((m, k)) < 0.08
        idx[hit] = rng.choice(np.array(GARBAGE + (rows, rows + 1, m + 5), dtype=np.int64), int(hit.sum()))
        if rows >= 4:
            idx[2, -1] = 2                                          # the row itself in the last slot
    P[rows:] = np.nan
    idx[rows:] = rng.integers(-3, m + 3, (m - rows, k))
    pts = np.full((m, cols), np.nan, dtype=dtype)
    pts[:, :3] = P
    return dict(points=pts, idx=idx, d2=d2, rows=rows)


def median_radius(c, share=0.5):
    """a radius that cuts about `share` of the live slots of a random cloud"""
    d2 = c["d2"][:c["rows"]]
    d2 = d2[np.isfinite(d2) & (d2 > 0)]
    return float(np.sqrt(np.quantile(d2, share))) if d2.size else 0.5


# ------------------------------------------------------------------ designed clouds
def cloud_of(points, idx, dtype, rows=None, **params):
    points = np.asarray(points, dtype=np.float64).astype(dtype)
    return dict(points=points, idx=np.asarray(idx, dtype=np.int64), rows=points.shape[0] if rows is None else rows, params=params)


def star(k, others):
    """idx (1 + others, k): row 0 names itself and every other row, the others name nobody"""
    idx = np.full((1 + others, k), -1, dtype=np.int64)
    idx[0, :1 + others] = np.arange(1 + others)
    return idx


BLOB = np.array([[0.9, 0.1, 0.05], [-0.8, 0.2, -0.1], [0.1, 0.5, 0.2], [-0.2, -0.6, 0.15], [0.3, 0.1, -0.3], [-0.1, -0.2, 0.25], [0.5, -0.3, -0.2],
                 [-0.6, 0.4, 0.1]])


def duplicates(dtype):
    """rows 0 and 1 are one point with one neighbourhood, in one order (each names the other first: q = 0): equal saliencies, bit for bit,
    and one keypoint, the lower row.  The other rows name nobody: their count is 1."""
    P = np.concatenate((np.zeros((2, 3)), BLOB))
    idx = np.full((10, 12), -1, dtype=np.int64)
    idx[0, :9] = [1] + list(range(2, 10))
    idx[1, :9] = [0] + list(range(2, 10))
    return cloud_of(P + np.array([0.25, -0.5, 1.0]), idx, dtype)


def planar(dtype):
    """an exactly planar neighbourhood in z = 0.5: every d_z is 0, so l0 = 0 exactly and nothing is salient"""
    P = BLOB.copy()
    P[:, 2] = 0.5
    return cloud_of(P, star(8, 7), dtype)


def collinear(dtype):
    """an exactly collinear neighbourhood along x: l0 = l1 = 0"""
    P = np.zeros((8, 3))
    P[:, 0] = BLOB[:, 0]
    P[:, 1], P[:, 2] = 0.25, -1.0
    return cloud_of(P, star(8, 7), dtype)


def counts(dtype):
    """row 0 has exactly min_neighbors = 5 members (itself and 4), row 5 one fewer; both neighbourhoods are salient otherwise"""
    P = np.concatenate((np.zeros((1, 3)), BLOB[:4], np.full((1, 3), 10.0), 10.0 + BLOB[:3]))
    idx = np.full((9, 6), -1, dtype=np.int64)
    idx[0, :5] = [0, 1, 2, 3, 4]
    idx[5, :4] = [5, 6, 7, 8]
    return cloud_of(P, idx, dtype, min_neighbors=5)


def ratio(dtype):
    """a diagonal covariance with l2 : l1 : l0 = 1 : 1/4 : 1/16 exactly (powers of two commute with the rounding of the division by the
    count): at gamma = 0.25 the ratio sits exactly at gamma and the strict test fails; at 0.5 it passes"""
    P = [[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 0.5, 0], [0, -0.5, 0], [0, 0, 0.25], [0, 0, -0.25]]
    return cloud_of(P, star(7, 6), dtype)


def only_itself(dtype):
    """row 0's slots all name row 0; row 1 names rows holding NaN and inf, and garbage: both are alone"""
    P = [[0.1, 0.2, 0.3], [1, 1, 1], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [2, 2, 2]]
    idx = np.full((6, 8), -1, dtype=np.int64)
    idx[0] = 0
    idx[1] = [2, 3, 4, 1 << 40, -7, 6, 7, 1]
    return cloud_of(P, idx, dtype, rows=5)


def non_finite(dtype):
    """row 0 names the blob and, between its rows, rows holding NaN and inf: they are no members, the blob alone decides"""
    P = np.concatenate((np.zeros((1, 3)), BLOB, [[np.nan, 0, 0], [0, np.inf, 0]]))
    idx = np.full((11, 12), -1, dtype=np.int64)
    idx[0, :11] = [9, 1, 2, 10, 3, 4, 5, 9, 6, 7, 8]
    clean = cloud_of(P[:9], star(12, 8), dtype)
    return cloud_of(P, idx, dtype), clean


def designed(dtype):
    """name -> cloud"""
    return {"duplicates": duplicates(dtype), "planar": planar(dtype), "collinear": collinear(dtype), "counts": counts(dtype), "ratio": ratio(dtype),
            "only_itself": only_itself(dtype), "non_finite": non_finite(dtype)[0]}


# ------------------------------------------------------------------ batches
def pad_batch(clouds, m=None, k=None):
    """clouds (dicts) -> points (N, m, c), idx (N, m, k) int64, rows (N,): pad rows hold NaN and slots of every kind, pad slots -1"""
    m = max(c["points"].shape[0] for c in clouds) if m is None else m
    k = max(c["idx"].shape[1] for c in clouds) if k is None else k
    cols, dtype = clouds[0]["points"].shape[1], clouds[0]["points"].dtype
    N = len(clouds)
    P = np.full((N, m, cols), np.nan, dtype=dtype)
    idx = np.full((N, m, k), -1, dtype=np.int64)
    rows = np.zeros(N, dtype=np.int32)
    for b, c in enumerate(clouds):
        mb, kb = c["idx"].shape
        P[b, :mb], idx[b, :mb, :kb], rows[b] = c["points"], c["idx"], c["rows"]
        idx[b, mb:] = np.arange((m - mb) * k).reshape(m - mb, k) % (m + 2) - 1
    return P, idx, rows


# ------------------------------------------------------------------ the covariance families of the accuracy test
FAMILIES = ("uniform", "planar 1e-3", "linear 1e-4", "2.5 km from the origin", "count 3")


def family(name, n, seed, members=12):
    """n neighbourhoods of `members` points (3 for "count 3") -> (n, members, 3) float64; member 0 is the row itself"""
    rng = np.random.default_rng(seed)
    if name == "count 3":
        members = 3
    Q = rng.uniform(-1.0, 1.0, (n, members, 3))
    if name == "planar 1e-3":
        Q[..., 2] *= 1e-3
    if name == "linear 1e-4":
        Q[..., 1:] *= 1e-4
    if name in ("planar 1e-3", "linear 1e-4"):                      # a random orientation per neighbourhood
        A = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
        Q = np.einsum("nij,nkj->nki", A, Q)
    if name == "2.5 km from the origin":
        Q = Q + np.array([2500.0, -1200.0, 300.0])
    return Q


def family_cloud(Q):
    """the neighbourhoods as one cloud: row r * members is the row itself and names the others -> (points, idx, the rows that have members)"""
    n, members, _ = Q.shape
    idx = np.full((n * members, members), -1, dtype=np.int64)
    first = np.arange(n) * members
    idx[first] = first[:, None] + np.arange(members)[None, :]
    return Q.reshape(-1, 3), idx, first


# ------------------------------------------------------------------ the cube-corner scene
CORNER_RADIUS = 0.6


def corner_scene(seed):
    """Three exactly planar faces of the cube [0, 4]^3 that meet at the origin, each a 16 x 16 jittered grid (step 0.25, jitter +-0.08): 768
    points -> (points (768, 3) float64, edge (768,) the distance to the nearest of the three edges, the coordinate axes)"""
    rng = np.random.default_rng(seed)
    g = (np.arange(16) + 0.5) * 0.25
    faces = []
    for axis in range(3):
        uv = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2) + rng.uniform(-0.08, 0.08, (256, 2))
        faces.append(np.insert(uv, axis, 0.0, axis=1))
    P = np.concatenate(faces)
    edge = np.stack([np.sqrt(P[:, (a + 1) % 3] ** 2 + P[:, (a + 2) % 3] ** 2) for a in range(3)], axis=1).min(axis=1)
    return P, edge


def family_covariances(name, n, seed):
    """the covariances of a family's neighbourhoods by the restatement -> (the six entries, each (n,), the trace (n,), the counts (n,))"""
    P, idx, first = family_cloud(family(name, n, seed))
    mem, q, _ = ir.members(P, ir.row_ok(P), idx, P.shape[0], None)
    count = 1 + mem.sum(axis=1)
    a = [x[first] for x in ir.covariance(mem, q, count)]
    return a, a[0] + a[3] + a[5], count[first]


def eigvalsh(a):
    """numpy.linalg.eigvalsh of the symmetric matrices with the six entries a -> (n, 3) ascending"""
    C = np.zeros((a[0].shape[0], 3, 3))
    for e, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        C[:, i, j] = C[:, j, i] = a[e]
    return np.linalg.eigvalsh(C)


U = 2.0 ** -53                      # the unit roundoff of float64
ACCURACY_ROWS = {"uniform": 12000, "planar 1e-3": 12000, "linear 1e-4": 12000, "2.5 km from the origin": 12000, "count 3": 200}
ACCURACY_SEED = 1


def accuracy():
    """name -> dict(B: the largest |lambda - eigvalsh| / (u trace) of the family, needed: the histogram of the sweeps after which every
    off-diagonal was exactly 0, a, lam, ref, trace, count) over ACCURACY_ROWS neighbourhoods per family"""
    out = {}
    for name, n in ACCURACY_ROWS.items():
        a, tr, count = family_covariances(name, n, ACCURACY_SEED)
        lam, needed = ir.eigenvalues(a, return_needed=True)
        ref = eigvalsh(a)
        out[name] = dict(B=float((np.abs(lam - ref).max(axis=1) / (U * tr)).max()), needed=np.bincount(needed, minlength=ir.SWEEPS + 2), a=a, lam=lam, ref=ref,
                         trace=tr, count=count)
    return out
