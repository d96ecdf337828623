"""Inputs that the CPU and the GPU tests of the whole-ball ISS keypoints share (tests/test_iss_ball_host.py, tests/test_gpu_iss_ball.py):
the layouts that exercise the coverage claim of dicp_amd/csrc/dicp_iss_ball.h, the designed clouds of tests/iss_cases.py as whole-ball
cases, and the scenes and the bound of the cross-check with the k-slot form.
"""
import numpy as np

import ball_clouds as bc
import iss_cases as ic
import iss_ref as ir

U = 2.0 ** -53


def cube(seed, m, dtype, scale=(1.0, 0.7, 0.45), offset=0.0):
    """m rows uniform in an anisotropic box (separated eigenvalues: salient rows)"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.0, 1.0, (m, 3)) * np.array(scale) + offset).astype(dtype)


def ball_radius(P, members):
    """a radius whose ball holds about `members` other rows of the finite rows of P, by the median of the distance to that neighbour"""
    Q = np.asarray(P, dtype=np.float64)[:, :3]
    Q = Q[np.isfinite(Q).all(-1)]
    D = np.sqrt(((Q[:, None, :] - Q[None, :, :]) ** 2).sum(-1))
    D.sort(axis=1)
    return float(np.median(D[:, min(members, Q.shape[0] - 1)]))


def rounds_down(dtype):
    """(points, radius): a radius whose float32 conversion is BELOW it, with rows exactly float32(radius) and the next float32 apart
    along every axis from a few rows of a dense box"""
    r = 0.06
    assert float(np.float32(r)) < r
    P = cube(11, 300, np.float64, scale=(0.15, 0.15, 0.15), offset=0.5)
    lo, up = np.float32(r), np.nextafter(np.float32(r), np.float32(1))
    extra = []
    for a in range(3):
        for d in (lo, up):
            e = np.zeros(3)
            e[a] = float(d)
            extra += [P[a] + e, P[a + 3] - e]
    return np.concatenate((P, np.array(extra))).astype(dtype), r


def layouts(dtype):
    """name -> (points (m, 3), salient radius, non-max radius): the layouts of the coverage claim"""
    out = {}
    L = bc.lattice(dtype)
    for r in bc.lattice_radii(dtype):
        out["lattice r=%.3f" % r] = (L, r, r)
    out["lattice scaled 0.1"] = (L * dtype(0.1), float(dtype(0.1)), float(dtype(0.1)) * 1.5)
    P, r = rounds_down(dtype)
    out["radius rounds down"] = (P, r, 0.75 * r)
    out["cube at 2500"] = (cube(12, 400, np.float64, scale=(0.3, 0.3, 0.3), offset=2500.0).astype(dtype), 0.05, 0.08)
    _, wall = bc.wall_pair(1, 500, dtype)
    out["wall"] = (wall, 0.08, 0.05)
    _, cl, cr = bc.cluster_pair(dtype)
    out["two clusters"] = (cl, cr * 0.3, cr * 0.2)
    far = cube(13, 300, np.float64, scale=(0.4, 0.4, 0.4))
    far[17] = [1.0e30, 0.0, 0.0] if dtype == np.float32 else [1.0e300, 0.0, 0.0]
    out["far outlier"] = (far.astype(dtype), 0.12, 0.12)
    flat = cube(14, 200, np.float64, scale=(0.4, 0.4, 0.4))
    big = 3.0e38 if dtype == np.float32 else 1.5e308
    flat[5], flat[6] = [big, 0.0, 0.0], [-big, 0.0, 0.0]
    out["flat"] = (flat.astype(dtype), 0.15, 0.1)
    return out


LAYOUT_NAMES = ("lattice r=1.000", "lattice r=1.500", "lattice r=2.000", "lattice r=1.414", "lattice r=2.236", "lattice scaled 0.1",
                "radius rounds down", "cube at 2500", "wall", "two clusters", "far outlier", "flat")


# ------------------------------------------------------------------ the designed clouds of iss_cases as whole-ball cases
def designed(dtype):
    """name -> (points, rows, radius, params): the index of the k-slot case named EVERY row of the neighbourhood, so a radius that holds
    the whole cloud (or, for `counts`, each of its two groups) gives the same member SETS; the order is the grid's."""
    d = ic.designed(dtype)
    out = {}
    for name in ("duplicates", "planar", "collinear", "ratio"):
        out[name] = (d[name]["points"], d[name]["rows"], 100.0, d[name]["params"])
    out["counts"] = (d["counts"]["points"], d["counts"]["rows"], 3.0, d["counts"]["params"])          # the groups are 17 apart
    P = np.array([[0.1, 0.2, 0.3], [50.0, 50.0, 50.0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.1, 0.2, 0.3]]).astype(dtype)
    out["only_itself"] = (P, 5, 1.0, {})                                        # rows 0 and 1 are alone; row 5 (a duplicate of 0) is past rows
    out["non_finite"] = (ic.non_finite(dtype)[0]["points"], 11, 100.0, {})
    return out


# ------------------------------------------------------------------ the cross-check with the k-slot form
K = 32


CROSS_RADIUS = 1.3


def cross_scene(seed, dtype):
    """(points (294, 3), radius): a jittered 7 x 7 x 6 lattice (step 1, jitter +-0.3) scaled by (1, 0.85, 0.7); every ball holds at most 31
    other rows, the median ball 11.  NOT a uniform random box: its sparse corners hold isolated cliques, rows that are each other's only
    members -- one member SET, hence one covariance up to rounding (the covariance does not depend on which member is the centre), and
    the suppression among them is decided by the last bits: 17 of 300 rows of such a box had to be left out, above the cap."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(7), np.arange(7), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    P = ((g + rng.uniform(-0.3, 0.3, g.shape)) * np.array([1.0, 0.85, 0.7])).astype(dtype)
    Q = P.astype(np.float64)
    D2 = ((Q[:, None, :] - Q[None, :, :]) ** 2).sum(-1)
    assert ((D2 <= (CROSS_RADIUS * 1.001) ** 2).sum(1) - 1).max() <= K - 1
    return P, CROSS_RADIUS


def eigenvalue_bound(radius, count_max, trace, dtype):
    """The bound of test_gpu_iss_ball.py's cross-check (derived in its docstring) on |eigenvalue (k-slot form) - eigenvalue (whole-ball
    form)| for neighbourhoods of at most count_max members inside `radius`, trace: the trace of the covariance (a bound on it)."""
    n = count_max + 3
    gamma = n * U / (1.0 - n * U)
    b = 48.0 * gamma * 1.01 * radius * radius + 2.0 * 27.5 * U * trace
    if np.dtype(dtype) == np.float32:
        b = b + 2.0 * 2.0 ** -24 * trace                                        # each output rounded once to float32
    return b


def excluded_rows(points, ref, radius, bound, idx, gamma21=0.975, gamma32=0.975, min_neighbors=5):
    """(m,) bool: the rows whose mask the cross-check does not compare -- a threshold test of the row, or a saliency comparison with one
    of its members, has no more margin than 2 * bound in the float64 reference `ref` (iss_ref's dict with idx its full index)"""
    lam = ref["eig"].astype(np.float64)
    margin = np.minimum(np.minimum(np.abs(gamma21 * lam[:, 2] - lam[:, 1]), np.abs(gamma32 * lam[:, 1] - lam[:, 0])), np.abs(lam[:, 0]))
    near = (ref["count"] >= min_neighbors) & (margin <= 2.0 * bound)           # (below min_neighbors the saliency is 0 on both sides)
    P, ok, rows = ir._cloud(np.asarray(points), None)
    mem, _, jc = ir.members(P, ok, idx, rows, radius)
    sal = ref["sal64"]
    close = mem & (np.abs(sal[jc] - sal[:, None]) <= 2.0 * bound) & ((sal[jc] > 0) | (sal[:, None] > 0))
    return near | close.any(axis=1) | (mem & near[jc]).any(axis=1)
