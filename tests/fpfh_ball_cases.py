"""Inputs that the CPU and the GPU tests of the whole-ball FPFH descriptor share (tests/test_fpfh_ball_host.py,
tests/test_gpu_fpfh_ball.py): random clouds with seeded unit normals and every kind of dead row, the wide-count lattice, the entries of
`at`, and the bound of the cross-check with the k-slot form.
"""
import numpy as np

import fpfh_cases as fc
import iss_ball_cases as ibc

U = 2.0 ** -53
DEAD_ROWS = (3, 9, 5, 7)            # a NaN coordinate, an inf coordinate, a zero normal, a NaN normal; row 11 is an exact duplicate of row 10


def normals(seed, m, dtype):
    """m seeded unit normals"""
    return fc.unit(np.random.default_rng(1000 + seed).standard_normal((m, 3))).astype(dtype)


def cloud(seed, m, dtype, cols=3, dead=False):
    """-> points (m, cols) from ibc.cube with NaN in the columns past 2, unit normals (m, 3); dead (m >= 12): the rows of DEAD_ROWS and
    the duplicate"""
    P = np.full((m, cols), np.nan, dtype=dtype)
    P[:, :3] = ibc.cube(seed, m, dtype)
    Nn = normals(seed, m, dtype)
    if dead:
        assert m >= 12
        P[3, 1], P[9, 0] = np.nan, np.inf
        Nn[5] = 0.0
        Nn[7, 2] = np.nan
        P[11] = P[10]
    return P, Nn


WIDE_RADIUS = 100.0
WIDE_CHANNELS = (5, 16, 27)         # theta = 0, alpha = 0, phi = 0: the middle bin of each feature


def wide_lattice(dtype):
    """a 20 x 20 unit lattice in z = 0 with normals +z: 399 pairs a row, all in the three channels of WIDE_CHANNELS"""
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 2)
    P = np.concatenate((g, np.zeros((400, 1))), axis=1).astype(dtype)
    Nn = np.zeros((400, 3), dtype=dtype)
    Nn[:, 2] = 1.0
    return P, Nn


def at_entries(m, rows, itype, seed=0):
    """a shuffled list of entries for a cloud of m rows of which `rows` count: live rows, the dead rows of `cloud`, duplicates, and the
    out-of-range values -1, m, rows, 2^31 - 1, -2^40 (int32: its clamp to the type)"""
    rng = np.random.default_rng(seed)
    live = rng.choice(rows, size=min(rows, 17), replace=False)
    at = np.concatenate((live, live[:4], [3, 5, 10, 11, 0, rows - 1, -1, m, rows, (1 << 31) - 1, -(1 << 40), -7, m + 5])).astype(np.int64)
    return fc.index_dtype(rng.permutation(at), itype)


def cross_bound(n, dtype):
    """The bound of test_gpu_fpfh_ball.py's cross-check (derived in its docstring) on |out (k-slot form) - out (whole-ball form)| for near
    lists of at most n rows"""
    k = n + 12
    b = 100.0 * 4.0 * (k * U / (1.0 - k * U))
    if np.dtype(dtype) == np.float32:
        b = b + 2.0 * 2.0 ** -24 * 200.0
    return b
