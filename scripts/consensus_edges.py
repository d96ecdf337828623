"""Measures the fit of a member list of csrc/dicp_compat2.h (the g++ host build) against the float64 numpy Kabsch and writes
profiles/r30_consensus_edges.txt: the largest normalised pose errors over lists of 3 .. 32 members, from which tests/compat2_ref.py takes
K_C and K_R (2 x).  CPU only.

    python scripts/consensus_edges.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import compat2_cases as cc  # noqa: E402
import compat2_ref as c2  # noqa: E402
import ransac_cases as rc  # noqa: E402

H = 4000
KS = (3, 4, 6, 10, 16, 32)


def main():
    lib = cc.build()
    lines = ["# fit of a member list: host build of csrc/dicp_compat2.h against float64 numpy Kabsch (np.linalg.svd, U diag(1, 1, det) V^T)",
             "# %d random lists of k distinct pairs per line from 512 pairs uniform in a unit cube; errors beyond the one rounding to T (u_T |v|), normalised:" % H,
             "#   eC = |dC| / g, eR = |dr| / (g s), g = 2^-53 s^2 / (w_2 + d w_3), s = the list's largest |coordinate|, w the singular values of the covariance W, d = sign(det W)",
             "# only lists with sigma_2 / sigma_1 >= %.1f count; share = the fraction that does" % c2.MIN_RATIO,
             "dtype    offset      noise   k    share   max eC     max eR"]
    worst_c = worst_r = 0.0
    for dtype in (np.float32, np.float64):
        for offset in (0.0, 2500.0):
            for noise in (0.0, 0.01, 1.0):
                for k in KS:
                    rng = np.random.default_rng(30 + k)
                    pairs = rc.cube_pairs(rng, 512, dtype, offset, noise)
                    lists = np.stack([rng.permutation(512)[:k] for _ in range(H)]).astype(np.int32)
                    _, poses = cc.header_fit(lib, pairs, lists)
                    eC, eR, ok = c2.pose_errors(poses, pairs, lists)
                    lines.append("%-8s %-11g %-7g %-4d %.3f   %-10.3g %-10.3g" % (np.dtype(dtype).name, offset, noise, k, ok.mean(), eC[ok].max(), eR[ok].max()))
                    worst_c, worst_r = max(worst_c, eC[ok].max()), max(worst_r, eR[ok].max())
    lines.append("largest eC %.3g, largest eR %.3g  ->  the tests' bounds: K_C = 2 x %.3g, K_R = 2 x %.3g (tests/compat2_ref.py holds K_C = %g, K_R = %g)"
                 % (worst_c, worst_r, worst_c, worst_r, c2.K_C, c2.K_R))
    out = os.path.join(ROOT, "profiles", "r30_consensus_edges.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
