"""Designed inputs that the CPU and the GPU tests of the whole-ball normals share (tests/test_normals_ball_host.py,
tests/test_gpu_normals_ball.py), each with the conditions that make it usable, computed on the numpy references alone.
"""
import numpy as np

import iss_ball_ref as ibr
import normals_ball_ref as nbr

# ------------------------------------------------------------------ the wavy sheet of the gradcheck
SHEET_RADIUS = 0.7


def sheet():
    """(40, 3) float64: a thin wavy sheet"""
    rng = np.random.default_rng(51)
    P = rng.uniform(-1, 1, (40, 3))
    P[:, 2] = 0.2 * P[:, 2] + 0.3 * np.sin(P[:, 0])
    return P


def border_distance(P, radius):
    """the smallest | |p_i - p_j| - radius | over the pairs of finite rows"""
    Q = np.asarray(P, dtype=np.float64)[:, :3]
    D = np.sqrt(((Q[:, None, :] - Q[None, :, :]) ** 2).sum(-1))
    return float(np.abs(D[np.triu_indices(Q.shape[0], 1)] - radius).min())


def relative_gaps(ref):
    """(lam_1 - lam_0) / trace of the rows of a forward_ref dict that have members"""
    lam = ref["lam"][ref["count"] > 0]
    return (lam[:, 1] - lam[:, 0]) / lam.sum(1)


def sheet_conditions():
    """-> (smallest count, largest count, smallest relative eigen gap, the nearest a pair comes to the ball's border): finite
    differences of 1e-6 cannot move a member and no row is at the tau cut when the last two are far above 1e-6 and 1e-12"""
    P = sheet()
    ref = nbr.forward_ref(P, SHEET_RADIUS)
    return int(ref["count"].min()), int(ref["count"].max()), float(relative_gaps(ref).min()), border_distance(P, SHEET_RADIUS)


# ------------------------------------------------------------------ the cluster lattice of the cross-check with the k-slot form
CLUSTER_RADIUS = 2.0
CLUSTER_SEEDS = (41, 42, 43)
CLUSTER_ROWS = 12


def clusters(seed, dtype, return_labels=False):
    """(300, 3): 25 clusters of exactly 12 rows on a 5 x 5 lattice of spacing 4, each uniform in a 1 x 1 x 0.2 box, rows permuted.  A
    box's diagonal is 1.43 < 2 and two boxes are at least 3 apart: by construction every ball of radius 2 holds exactly its cluster and
    every pair stays 0.57 away from the border."""
    rng = np.random.default_rng(seed)
    centres = np.stack(np.meshgrid(np.arange(5) * 4.0, np.arange(5) * 4.0, indexing="ij"), -1).reshape(-1, 2)
    P = rng.uniform(0.0, 1.0, (25, CLUSTER_ROWS, 3)) * np.array([1.0, 1.0, 0.2])
    P[:, :, :2] += centres[:, None, :]
    labels = np.repeat(np.arange(25), CLUSTER_ROWS)
    perm = rng.permutation(25 * CLUSTER_ROWS)
    P, labels = P.reshape(-1, 3)[perm].astype(dtype), labels[perm]
    return (P, labels) if return_labels else P


def cluster_conditions(seed, dtype):
    """-> (every ball is exactly its cluster, smallest count, largest count, smallest relative gap, nearest pair to the border)"""
    P, labels = clusters(seed, dtype, return_labels=True)
    mem = ibr.members_brute(P, None, CLUSTER_RADIUS)
    same = labels[:, None] == labels[None, :]
    np.fill_diagonal(same, False)
    ref = nbr.forward_ref(P, CLUSTER_RADIUS)
    return bool(np.array_equal(mem, same)), int(ref["count"].min()), int(ref["count"].max()), float(relative_gaps(ref).min()), \
        border_distance(P, CLUSTER_RADIUS)
