"""Inputs shared by tests/test_match_host.py and tests/test_gpu_match.py.  A plain module (no fixtures)."""
import numpy as np


def rotation(angle, axis):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def end_to_end(seed=0, n=500, m=600, D=32, dtype=np.float32):
    """Descriptors and points with a known answer: fy standard normal, fx = fy[gt] + 0.05 noise for a random injection gt, about 20 % of the
    x rows replaced by fresh random descriptors (gt = -1 there); points x = R^-1 (y[gt] - t) + 0.005 noise.
    -> dict(fx, fy, x, y, gt, R, t)"""
    rng = np.random.default_rng(seed)
    fy = rng.standard_normal((m, D))
    gt = rng.permutation(m)[:n]
    fx = fy[gt] + 0.05 * rng.standard_normal((n, D))
    replaced = rng.random(n) < 0.2
    fx[replaced] = rng.standard_normal((int(replaced.sum()), D))
    R = rotation(0.5, [0.3, -0.5, 0.8])
    t = np.array([0.3, -0.2, 0.1])
    y = rng.uniform(-0.5, 0.5, (m, 3))
    x = (y[gt] - t) @ R + 0.005 * rng.standard_normal((n, 3))      # row form of R^T (y - t)
    return dict(fx=fx.astype(dtype), fy=fy.astype(dtype), x=x.astype(dtype), y=y.astype(dtype), gt=np.where(replaced, -1, gt).astype(np.int64), R=R, t=t)


def kabsch(x, y, w):
    """float64 numpy SVD Kabsch: (C, r) minimising sum w |C x + r - y|^2, C = U diag(1, 1, det U det V) V^T"""
    w = w / w.sum()
    mx, my = (w[:, None] * x).sum(0), (w[:, None] * y).sum(0)
    H = ((y - my) * w[:, None]).T @ (x - mx)
    U, _, Vt = np.linalg.svd(H)
    C = U @ np.diag([1.0, 1.0, np.linalg.det(U) * np.linalg.det(Vt)]) @ Vt
    return C, my - C @ mx
