"""Measures the minimal-sample fit of csrc/dicp_ransac.h (the g++ host build) against the float64 numpy Kabsch and writes
profiles/r26_ransac_edges.txt: the largest normalised pose errors, from which tests/ransac_cases.py takes K_C and K_R (16 x).  CPU only.

    python scripts/ransac_edges.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ransac_cases as rc  # noqa: E402

H = 20000


def main():
    lib = rc.build()
    lines = ["# minimal-sample fit: host build of csrc/dicp_ransac.h against float64 numpy Kabsch (np.linalg.svd, U diag(1, 1, det) V^T)",
             "# %d triples per line from 512 pairs uniform in a unit cube; errors beyond the one rounding to T (u_T |v|), normalised:" % H,
             "#   eC = |dC| / g, eR = |dr| / (g s), g = 2^-53 s^2 / w_2, s = the triple's largest |coordinate|, w_2 the second singular value of the covariance",
             "# only triples with sigma_2 / sigma_1 >= %.1f count; share = the fraction that does" % rc.MIN_RATIO,
             "dtype    offset      noise   share   max eC     max eR     max |dC|   max |dr|"]
    worst_c = worst_r = 0.0
    for dtype in (np.float32, np.float64):
        for offset in (0.0, 2500.0):
            for noise in (0.0, 0.01, 1.0):
                rng = np.random.default_rng(26)
                pairs = rc.cube_pairs(rng, 512, dtype, offset, noise)
                smp, _, poses = rc.header_hypotheses(lib, pairs, H, seed=7)
                eC, eR, ok = rc.pose_errors(poses, pairs, smp)
                tri = pairs[smp].astype(np.float64)
                ref = rc.rr.kabsch(tri[:, :, :3], tri[:, :, 3:])[0]
                d = np.abs(poses.astype(np.float64) - ref)[ok]
                lines.append("%-8s %-11g %-7g %.3f   %-10.3g %-10.3g %-10.3g %-10.3g" % (np.dtype(dtype).name, offset, noise, ok.mean(), eC[ok].max(), eR[ok].max(),
                                                                                     d[:, :9].max(), d[:, 9:].max()))
                worst_c, worst_r = max(worst_c, eC[ok].max()), max(worst_r, eR[ok].max())
    lines.append("largest eC %.3g, largest eR %.3g  ->  the tests' bounds: K_C = 16 x %.3g, K_R = 16 x %.3g (tests/ransac_cases.py holds K_C = %g, K_R = %g)"
                 % (worst_c, worst_r, worst_c, worst_r, rc.K_C, rc.K_R))
    out = os.path.join(ROOT, "profiles", "r26_ransac_edges.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
