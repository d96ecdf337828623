"""The clouds that the farthest-point-sampling tests share (tests/test_fps_host.py without a GPU, tests/test_gpu_fps.py on one): each is built
to make one part of the rule matter -- exact ties, duplicates, rows that are no candidates, overflow, roundings that the two dtypes make
differently.  A plain module (no fixtures): the tests put this directory on sys.path and import it."""
import numpy as np


def random_cloud(n, c=3, dtype=np.float32, seed=0, scale=10.0):
    return (np.random.default_rng(seed).standard_normal((n, c)) * scale).astype(dtype)


def lattice_cloud(n, dtype=np.float32, seed=1, c=3):
    """n rows drawn from {0, 1, 2, 3}^3: 64 positions, so most rows are duplicates and every distance is an exact small integer (ties)"""
    p = np.random.default_rng(seed).integers(0, 4, (n, c)).astype(dtype)
    return p


def repeated_point(n=200, dtype=np.float32):
    return np.tile(np.array([[1.5, -2.25, 0.75]], dtype=dtype), (n, 1))


def grid_cloud(side=17, dtype=np.float32, seed=2):
    """a regular side^3 grid in shuffled order"""
    g = np.stack(np.meshgrid(*([np.arange(side)] * 3), indexing="ij"), -1).reshape(-1, 3).astype(dtype)
    return g[np.random.default_rng(seed).permutation(g.shape[0])]


def nonfinite_cloud(n=700, dtype=np.float32, seed=3, c=3):
    """NaN, +inf and -inf rows scattered through a random cloud; row 5 (a start) and the last 9 rows are non-finite"""
    rng = np.random.default_rng(seed)
    p = random_cloud(n, c, dtype, seed)
    bad = np.unique(np.concatenate((rng.choice(n, n // 5, replace=False), [5], np.arange(n - 9, n))))
    vals = np.array([np.nan, np.inf, -np.inf], dtype=dtype)
    p[bad, rng.integers(0, 3, bad.size)] = vals[rng.integers(0, 3, bad.size)]
    return p


def overflow_cloud(n=500, seed=4):
    """float32 coordinates near 1e20 with both signs: d2 overflows to +inf between most pairs"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], (n, 3)) * rng.uniform(0.2e20, 1.5e20, (n, 3))).astype(np.float32)


def sphere_cloud(n=2000, seed=5):
    """points on the sphere of radius 1 around (2500, 2500, 0), stored in float32, in a thin band round its equator: groups of 4 rows share
    their (x, y) and differ in z by ~1e-5.  From any pick the rows of a group are near-ties -- their d2 differ by ~1e-10, far below the
    float32 spacing of d2 at this offset but not below float64's: float32 takes the lowest index of a group, float64 its true farthest row"""
    rng = np.random.default_rng(seed)
    th = np.repeat(rng.uniform(0.0, 2.0 * np.pi, (n + 3) // 4), 4)[:n]
    v = np.stack((np.cos(th), np.sin(th), rng.standard_normal(n) * 1e-5), 1)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v + np.array([2500.0, 2500.0, 0.0])).astype(np.float32)
