"""CPU-only figures behind the FPFH tests, written to profiles/r27_fpfh_edges.txt (no GPU, no library: tests/fpfh_ref.py alone).

1  the half-plane rule of the theta bin against floor(11 (atan2 + pi) / 2 pi) on random pairs: disagreements, and how close to an edge;
2  invariance: a rigidly moved, row-permuted copy of the scene (float64, m = 1500, k = 24, radius 0.6), the share of rows whose nearest
   descriptor is the row they came from;
3  the end-to-end scene of tests/test_gpu_fpfh.py (m = 1500, the source an 85 % subset, 1 rad about a nearly vertical axis, 2 mm noise;
   numpy PCA normals facing each scan's viewpoint; radius 0.8, k = 32): the share of mutual matches within 0.15 of the true row -- the
   figure the GPU test halves.

    python scripts/fpfh_edges.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fpfh_cases as fc  # noqa: E402
import fpfh_ref as fr  # noqa: E402


def ball_idx(P, radius, k):
    """ball_query(P, P, radius, k)'s index: the nearest k rows within the radius, the row itself among them"""
    d2, idx = fr.knn_self(P, k)
    return np.where(d2 <= radius * radius, idx, -1)


def main():
    lines = []
    rng = np.random.default_rng(0)
    n = 200000
    P = rng.uniform(-1, 1, (2, n, 3))
    Nn = fc.unit(rng.standard_normal((2, n, 3)))
    f = fr.pair_features(P[0], Nn[0], P[1], Nn[1])
    want, dist = fr.bin_theta_atan2(f["cos"], f["sin"])
    got = fr.bin_theta(f["cos"], f["sin"])
    ok = f["frame"]
    lines.append("theta bin, half-plane rule against the atan2 form: %d random pairs, %d disagreements; closest to an edge %.3g bins"
                 % (int(ok.sum()), int((got[ok] != want[ok]).sum()), float(dist[ok].min())))

    m = 1500
    S = fc.scene(0, m)
    Ns = fc.normals_np(S, 16, fc.VIEWPOINT)
    mv = fc.moved_copy(S, seed=0)
    f0, c0 = fr.fpfh_ref(S, Ns, fr.knn_self(S, 24)[1], radius=0.6)
    f1, c1 = fr.fpfh_ref(mv["x"], Ns[mv["src"]] @ mv["R"].T, fr.knn_self(mv["x"], 24)[1], radius=0.6)
    to, _ = fc.nearest_rows(f1, f0)
    lines.append("invariance, m = 1500, k = 24, radius 0.6, float64: nearest descriptor is the true row for %.4f of the rows; "
                 "bin counts equal on %.4f; %d distinct descriptors; %.1f pairs per row"
                 % (float((to == mv["src"]).mean()), float((c0[mv["src"]] == c1).all(axis=1).mean()), len(np.unique(f0, axis=0)), c0.sum() / 3.0 / m))

    for keep in (0.85, 0.70):
        mv = fc.moved_copy(S, seed=0, keep=keep, angle=1.0, noise=0.002, axis=fc.E2E_AXIS)
        X = mv["x"]
        Nx = fc.normals_np(X, 16, fc.VIEWPOINT @ mv["R"].T + mv["t"])
        fy, _ = fr.fpfh_ref(S.astype(np.float32), Ns.astype(np.float32), ball_idx(S, 0.8, 32), radius=0.8)
        fx, _ = fr.fpfh_ref(X.astype(np.float32), Nx.astype(np.float32), ball_idx(X, 0.8, 32), radius=0.8)
        to, mutual = fc.nearest_rows(fx, fy)
        err = np.linalg.norm(S[to] - S[mv["src"]], axis=1)
        lines.append("end to end, m = 1500, source %.0f %% of the rows, 1 rad, 2 mm noise, radius 0.8, k = 32, float32: %d mutual matches of %d rows, "
                     "%.3f of them within 0.15 of the true row (all nearest rows: %.3f)"
                     % (100 * keep, int(mutual.sum()), X.shape[0], float((err[mutual] <= 0.15).mean()), float((err <= 0.15).mean())))
    out = os.path.join(ROOT, "profiles", "r27_fpfh_edges.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
