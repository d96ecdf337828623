"""CPU-only figures behind the whole-ball FPFH tests, written to profiles/r36_fpfh_ball_edges.txt (no GPU, no library: the numpy
references tests/fpfh_ref.py, tests/fpfh_ball_ref.py and tests/iss_ball_ref.py alone), measured before any threshold of
tests/test_gpu_fpfh_ball.py was fixed.

The end-to-end scene of tests/test_gpu_fpfh.py (tests/fpfh_cases.py: scene(0, 1500), the source an 85 % subset turned by 1 rad about a
nearly vertical axis, 2 mm noise, float32; numpy PCA normals over 16 rows facing each scan's viewpoint), at radius 0.8 and 1.2:

1  the rows in a ball; the share of mutual matches within 0.15 of the true row with the k-slot form (the 32 nearest rows of the ball, the
   row itself among them) and with every row of the ball -- the second figure at radius 1.2 is the one the GPU test halves;
2  the whole-ball ISS keypoints of both clouds (radii 0.8 / 0.4) and, with whole-ball descriptors AT them, the mutual matches among the
   keypoints and how many are within 0.15 of the true row.

    python scripts/fpfh_ball_edges.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fpfh_ball_ref as fbr  # noqa: E402
import fpfh_cases as fc  # noqa: E402
import fpfh_ref as fr  # noqa: E402
import iss_ball_ref as ibr  # noqa: E402

from fpfh_edges import ball_idx  # noqa: E402


def main():
    lines = []
    S = fc.scene(0, 1500)
    mv = fc.moved_copy(S, seed=0, keep=0.85, angle=1.0, noise=0.002, axis=fc.E2E_AXIS)
    X = mv["x"]
    Ns = fc.normals_np(S, 16, fc.VIEWPOINT)
    Nx = fc.normals_np(X, 16, fc.VIEWPOINT @ mv["R"].T + mv["t"])
    S32, X32, Ns32, Nx32 = (a.astype(np.float32) for a in (S, X, Ns, Nx))
    truth = S[mv["src"]]

    def share(fx, fy, rows_x=None, rows_y=None):
        """mutual matches of fx[rows_x] in fy[rows_y], and how many name a row within 0.15 of the true one"""
        rows_x = np.arange(fx.shape[0]) if rows_x is None else rows_x
        rows_y = np.arange(fy.shape[0]) if rows_y is None else rows_y
        to, mutual = fc.nearest_rows(fx[rows_x], fy[rows_y])
        err = np.linalg.norm(S[rows_y[to]] - truth[rows_x], axis=1)
        return int(mutual.sum()), int((err[mutual] <= 0.15).sum())

    kx = np.flatnonzero(ibr.keypoints_ball_ref(X32, 0.8, 0.4)["mask"])
    ky = np.flatnonzero(ibr.keypoints_ball_ref(S32, 0.8, 0.4)["mask"])
    lines.append("whole-ball ISS keypoints (radii 0.8 / 0.4): %d of %d source rows, %d of %d target rows" % (kx.size, X.shape[0], ky.size, S.shape[0]))
    for radius in (0.8, 1.2):
        slot_y, _ = fr.fpfh_ref(S32, Ns32, ball_idx(S, radius, 32), radius=radius)
        slot_x, _ = fr.fpfh_ref(X32, Nx32, ball_idx(X, radius, 32), radius=radius)
        by, bx = fbr.fpfh_ball_ref(S32, Ns32, radius), fbr.fpfh_ball_ref(X32, Nx32, radius)
        rows = by["cnt"][:, :fr.BINS].sum(axis=1)
        n_k, ok_k = share(slot_x, slot_y)
        n_b, ok_b = share(bx["out"], by["out"])
        lines.append("radius %.1f, float32: rows in a ball (pairs of a target row) mean %.0f, max %d; k-slot form (32 nearest): %d mutual matches, "
                     "%.3f within 0.15 of the true row; every row of the ball: %d mutual matches, %.3f within 0.15"
                     % (radius, rows.mean(), rows.max(), n_k, ok_k / n_k, n_b, ok_b / n_b))
        n_kp, ok_kp = share(bx["out"], by["out"], kx, ky)
        lines.append("radius %.1f, whole-ball descriptors at the ISS keypoints: %d mutual matches, %d of them within 0.15 of the true row"
                     % (radius, n_kp, ok_kp))
    out = os.path.join(ROOT, "profiles", "r36_fpfh_ball_edges.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
