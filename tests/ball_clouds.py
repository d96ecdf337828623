"""The clouds of the ball_query tests (tests/test_ball_host.py on the CPU, tests/test_gpu_ball.py on the GPU): numpy, deterministic."""
import numpy as np

RANDOM_SHAPES = ((1, 1), (2, 257), (700, 5000), (3000, 300))
RANDOM_RADII = (0.02, 0.05, 0.1, 0.2, 2.0)
KS = (1, 8, 32)


def random_pair(n, m, dtype, seed=0):
    """n queries and m rows uniform in the unit cube"""
    rng = np.random.default_rng(1000 * seed + 7 * n + m)
    return rng.random((n, 3)).astype(dtype), rng.random((m, 3)).astype(dtype)


def lattice(dtype):
    """the integer lattice {-3 .. 3}^3: 343 rows, row 171 the centre"""
    g = np.arange(-3, 4)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(dtype)


def lattice_radii(dtype):
    return [1.0, 1.5, 2.0, float(np.sqrt(dtype(2))), float(np.sqrt(dtype(5)))]


def lattice_cases(dtype):
    """(name, x, y, radius): the lattice against itself -- plain, scaled so that every point lies on a cell border, at negative
    coordinates, and (float32) 2.5 km and 10^6 from the origin"""
    L = lattice(dtype)
    out = [("lattice r=%r" % r, L, L, r) for r in lattice_radii(dtype)]
    for r in (0.25, 0.1):
        out.append(("lattice scaled by %r" % r, L * dtype(r), L * dtype(r), float(dtype(r))))
    out.append(("lattice at -100", L - dtype(100), L - dtype(100), 1.0))
    out.append(("lattice at -100 r=2", L - dtype(100), L - dtype(100), 2.0))
    if dtype == np.float32:
        for off in (2500.0, 1.0e6):
            for r in (1.0, 2.0):
                out.append(("lattice at %g r=%g" % (off, r), L + dtype(off), L + dtype(off), r))
    return out


def wall_pair(n, m, dtype, seed=3):
    """a wall perpendicular to x (every row at x = 0.5) and queries within 0.06 of it"""
    rng = np.random.default_rng(seed)
    y = rng.random((m, 3))
    y[:, 0] = 0.5
    x = rng.random((n, 3))
    x[:, 0] = 0.5 + (rng.random(n) - 0.5) * 0.12
    return x.astype(dtype), y.astype(dtype)


def cluster_pair(dtype, seed=4):
    """two clusters near (0, 0, 0) and (2e6, 2e6, 2e6): extent / radius needs more than 64 key bits.  -> x, y, radius"""
    rng = np.random.default_rng(seed)
    spread, radius = (1.0, 0.5) if dtype == np.float32 else (2.0e-3, 1.0e-3)
    a = (rng.random((250, 3)) - 0.5) * spread
    b = (rng.random((250, 3)) - 0.5) * spread + 2.0e6
    y = np.concatenate([a, b]).astype(dtype)
    x = np.concatenate([a[:60] + spread * 0.05, b[:60] - spread * 0.05, y[:20]]).astype(dtype)
    return x, y, radius


def degenerate_cases(dtype):
    """(name, x, y, radius)"""
    rng = np.random.default_rng(5)
    out = []
    pt = np.array([[0.3, -1.7, 2.2]])
    out.append(("300 copies", np.concatenate([pt, pt + 0.01, pt + 1.0]).astype(dtype), np.repeat(pt, 300, 0).astype(dtype), 0.05))
    t = np.linspace(0.0, 1.0, 1500)
    z = np.zeros_like(t)
    q = rng.random((200, 3)) * np.array([0.02, 0.02, 1.0])
    out.append(("line along z", q.astype(dtype), np.stack([z, z, t], 1).astype(dtype), 0.01))
    out.append(("line along x", q[:, ::-1].astype(dtype), np.stack([t, z, z], 1).astype(dtype), 0.01))
    wx, wy = wall_pair(400, 3000, dtype)
    out.append(("wall", wx, wy, 0.05))
    cx, cy, cr = cluster_pair(dtype)
    out.append(("two clusters", cx, cy, cr))
    _, y = random_pair(1, 500, dtype, seed=6)
    far = np.array([[1.0e3, 0.5, 0.5], [0.5, -50.0, 0.5], [0.5, 0.5, 1.0e30], [-1.0e30, -1.0e30, -1.0e30], [1.05, 0.5, 0.5], [0.5, 0.5, 0.5]])
    out.append(("far queries", far.astype(dtype), y, 0.1))
    ox, oy = random_pair(400, 3000, np.float64, seed=7)
    out.append(("cube at 2500", (ox + 2500.0).astype(dtype), (oy + 2500.0).astype(dtype), 0.05))      # float32: p +- R rounds coarser than the cells
    if dtype == np.float32:
        out.append(("underflow", np.zeros((1, 3), dtype), np.array([[0, 0, 0], [1e-23, 0, 0], [1e-3, 0, 0]], dtype), 1e-25))
    return out


def nonfinite_pair(dtype, seed=8):
    """x (300, 3) and y (900, 3) in the unit cube with NaN / +inf / -inf rows in both"""
    x, y = random_pair(300, 900, dtype, seed=seed)
    y[5] = np.nan
    y[17, 1] = np.inf
    y[400, 2] = -np.inf
    y[899, 0] = np.nan
    x[0, 0] = np.nan
    x[7] = np.inf
    x[150, 2] = -np.inf
    return x, y
