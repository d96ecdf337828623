"""CPU-only figures behind the ISS tests, written to profiles/r31_iss_edges.txt (no GPU, no library: tests/iss_ref.py alone).

1  the Jacobi eigenvalues of the restatement against numpy.linalg.eigvalsh over the families of tests/iss_cases.py: B, the largest
   |lambda - eigvalsh| / (u trace) per family -- tests/test_iss_host.py asserts twice the largest -- and after how many sweeps every
   off-diagonal entry was exactly 0;
2  whether any sweep after the fourth changes a bit of the eigenvalues, on random, graded, near-identity and nearly degenerate matrices;
3  the cube-corner scene of tests/test_gpu_iss.py, seeds 0 to 5: the largest ball, keypoints, where they lie;
4  the end-to-end scene of tests/test_gpu_iss.py: keypoints, mutual matches and true matches with tests/fpfh_ref.py's descriptors.

    python scripts/iss_edges.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fpfh_cases as fc  # noqa: E402
import fpfh_ref as fr  # noqa: E402
import iss_cases as ic  # noqa: E402
import iss_ref as ir  # noqa: E402


def ball_idx(P, radius, k):
    """ball_query(P, P, radius, k)'s index: the nearest k rows within the radius, the row itself among them"""
    d2, idx = ir.knn_self(P, k)
    return np.where(d2 <= radius * radius, idx, -1)


def six(M):
    return [M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]]


def main():
    lines = []
    acc = ic.accuracy()
    for name, v in acc.items():
        lines.append("eigenvalues against eigvalsh, %-24s %5d neighbourhoods: B = %.2f; sweeps until every off-diagonal is exactly 0 (0, 1, ..., 6, more): %s"
                     % (name + ",", v["lam"].shape[0], v["B"], [int(x) for x in v["needed"]]))
    lines.append("the largest B: %.2f; tests/test_iss_host.py asserts B <= 27.5" % max(v["B"] for v in acc.values()))

    rng = np.random.default_rng(0)
    n = 400000
    fams = {"gaussian entries": [rng.standard_normal(n) for _ in range(6)]}
    sc = 10.0 ** rng.uniform(-8, 0, (n, 3))
    M = rng.standard_normal((n, 3, 3))
    fams["graded over 16 decades"] = six((M + M.transpose(0, 2, 1)) * sc[:, :, None] * sc[:, None, :])
    for eps in (1e-3, 1e-12):
        S = rng.standard_normal((n, 3, 3))
        fams["identity + %g S" % eps] = six(np.eye(3)[None] + eps * (S + S.transpose(0, 2, 1)))
    A = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    D = np.stack((np.ones(n), 1 + 1e-8 * rng.standard_normal(n), rng.uniform(0, 3, n)), 1)
    fams["two eigenvalues 1e-8 apart"] = six(np.einsum("nij,nj,nkj->nik", A, D, A))
    for name, a in fams.items():
        l3, l4, l5, l6 = (ir.eigenvalues(a, s) for s in (3, 4, 5, 6))
        _, needed = ir.eigenvalues(a, 8, return_needed=True)
        lines.append("sweeps, %-28s %d matrices: eigenvalues differ between 3 and 4 sweeps on %d, 4 and 5 on %d, 5 and 6 on %d; "
                     "sweeps until exact zeros (0 .. 8, more): %s"
                     % (name + ",", n, int((l3 != l4).any(1).sum()), int((l4 != l5).any(1).sum()), int((l5 != l6).any(1).sum()), [int(x) for x in np.bincount(needed, minlength=10)]))

    for seed in range(6):
        P, edge = ic.corner_scene(seed)
        ball = int((((P[:, None] - P[None]) ** 2).sum(-1) <= ic.CORNER_RADIUS ** 2).sum(1).max())
        r = ir.keypoints_ref(P, ball_idx(P, ic.CORNER_RADIUS, 32), None, ic.CORNER_RADIUS, ic.CORNER_RADIUS)
        kp = np.flatnonzero(r["mask"])
        lines.append("corner scene, seed %d: the largest ball holds %d rows; %d salient rows, %d of them farther than 0.6 from every edge; %d keypoints, "
                     "the farthest from an edge %.3f, the nearest to the corner %.3f"
                     % (seed, ball, int((r["sal64"] > 0).sum()), int((r["sal64"][edge > ic.CORNER_RADIUS] != 0).sum()), kp.size, float(edge[kp].max()),
                        float(np.linalg.norm(P[kp], axis=1).min())))

    S = fc.scene(0, 1500)
    Ns = fc.normals_np(S, 16, fc.VIEWPOINT)
    mv = fc.moved_copy(S, seed=0, keep=0.85, angle=1.0, noise=0.002, axis=fc.E2E_AXIS)
    X = mv["x"]
    Nx = fc.normals_np(X, 16, fc.VIEWPOINT @ mv["R"].T + mv["t"])
    fy, _ = fr.fpfh_ref(S.astype(np.float32), Ns.astype(np.float32), ball_idx(S, 0.8, 32), radius=0.8)
    fx, _ = fr.fpfh_ref(X.astype(np.float32), Nx.astype(np.float32), ball_idx(X, 0.8, 32), radius=0.8)
    for rs, rn in ((0.8, 0.8), (0.8, 0.4), (0.6, 0.3)):
        iy = np.flatnonzero(ir.keypoints_ref(S.astype(np.float32), ball_idx(S, max(rs, rn), 32), None, rs, rn)["mask"])
        ix = np.flatnonzero(ir.keypoints_ref(X.astype(np.float32), ball_idx(X, max(rs, rn), 32), None, rs, rn)["mask"])
        to, mutual = fc.nearest_rows(fx[ix], fy[iy])
        err = np.linalg.norm(S[iy[to]] - S[mv["src"][ix]], axis=1)
        lines.append("end to end, m = 1500, source 85 %% of the rows, salient radius %.1f, non-max radius %.1f, k = 32, float32: %d and %d keypoints, "
                     "%d mutual matches, %d of them within 0.15 of the true row" % (rs, rn, ix.size, iy.size, int(mutual.sum()), int((err[mutual] <= 0.15).sum())))
    out = os.path.join(ROOT, "profiles", "r31_iss_edges.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
