"""The recovery runs of gnc_correspondences on the g++ build of csrc/dicp_gnc.h (no GPU): the rotation error against the truth of every
case of tests/gnc_cases.recovery_cases() under both losses -- the largest per family, doubled, is the limit the tests assert
(gnc_cases.LIMIT_COMPAT / LIMIT_RANSAC) --, the least-squares error on the same matches, whether TLS ends with weights > 0 exactly on
the true pairs, and the same runs at 120 and 60 true pairs of 600, where GNC alone starts to lose clouds.

    python scripts/gnc_edges.py > profiles/r32_gnc_edges.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import compat_ref as cr  # noqa: E402
import gnc_cases as gc  # noqa: E402
import ransac_ref as rr  # noqa: E402


def run(lib, name, case, thr):
    ls = gc.least_squares_error(case)
    errs = []
    for loss in ("tls", "gm"):
        h = gc.header_call(lib, case["x"], case["y"], case["idx"], thr, loss)
        err = rr.rotation_error(h["pose_last"][:9], case["C"])
        errs.append(err)
        exact = bool(np.array_equal(h["weights"] > 0, case["truth"]))
        print("%-22s %-3s rounds %3d status %d mu %-9.4g rotation error %.3e rad   least squares %.3e rad   weights > 0 exactly on truth: %s"
              % (name, loss, h["rounds"], h["status"], h["mu"], err, ls, exact))
    return max(errs)


def main():
    lib = gc.build()
    worst = {}
    print("# the asserted runs (tests/gnc_cases.recovery_cases): float32 inputs, growth 1.4, iterations 128")
    for name, case, thr, _ in gc.recovery_cases():
        fam = name.split()[0]
        worst[fam] = max(worst.get(fam, 0.0), run(lib, name, case, thr))
    for fam, v in worst.items():
        print("# largest error of family %-6s %.3e rad -> limit %.3e rad" % (fam, v, 2 * v))
    print("# fewer inliers (not asserted: GNC alone is for ratios of about 30 % and up)")
    for k in (120, 60):
        lost = 0
        for s in range(5):
            lost += run(lib, "compat k=%d seed %d" % (k, s), cr.recovery_case(s, inliers=k), 0.05) > 1e-2
        print("# k = %d: %d of 5 clouds lost (an error above 1e-2 rad under either loss)" % (k, lost))


if __name__ == "__main__":
    main()
