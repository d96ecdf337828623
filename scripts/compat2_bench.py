"""Times second_order_compatibility's stages, prune_correspondences(order=2) beside order=1 and consensus_correspondences beside
ransac_correspondences on one GPU, and writes profiles/r30_compat2_bench.txt.  Medians of 5 (every sample is printed): 32 clouds x
{2048, 4096, 16384} matches, float32 and float64, 10 % inliers (scripts/compat_bench.py's generator); then the poses found at 10 %, 5 % and
1 % inliers.  Every (matches, dtype) step is a child process of its own under a time limit; the first failure ends the run.

    python scripts/compat2_bench.py [--out profiles/r30_compat2_bench.txt] [--quick]
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from compat_bench import WAVE_ISSUE_PER_S, make, timed  # noqa: E402
from dicp_amd import _lib  # noqa: E402
from dicp_amd import match as M  # noqa: E402
from dicp_amd._pairs import _live_pairs  # noqa: E402
from dicp_amd._ops import _DT, _p  # noqa: E402

N, THR = 32, 0.02
OPS_PER_WORD_PAIR = 4       # two 32-bit ANDs and two accumulating 32-bit popcounts per pair of 64-bit words
STEP_LIMIT_S = 240


def stage_times(x, y, idx, lines):
    n, dt, dev = x.shape[1], x.dtype, x.device
    code = _DT[dt]
    W = (n + 63) // 64
    pk = _live_pairs(x, y, idx, None)
    pairs, P = pk.pairs, pk.P
    adj = torch.empty((N, n, W), dtype=torch.int64, device=dev)
    dp = torch.empty((N, n), dtype=torch.int32, device=dev)
    d2 = torch.empty((N, n), dtype=torch.int64, device=dev)
    rank = torch.empty((N, n), dtype=torch.int32, device=dev)
    s2 = torch.empty((N, n), dtype=dt, device=dev)
    seedpos = torch.empty((N, 64), dtype=torch.int32, device=dev)
    mem = torch.empty((N, 64, 16), dtype=torch.int32, device=dev)
    poses = torch.empty((N, 64, 12), dtype=dt, device=dev)

    def bits():
        _lib.call("dicp_compat2_bits", dev, code, _p(pairs), _p(P), N, n, THR, 0.0, _p(adj), _p(dp), _p(d2))

    def common():
        _lib.call("dicp_zero", dev, _p(d2), d2.numel() * 8)
        _lib.call("dicp_compat2_common", dev, _p(adj), _p(P), N, n, _p(d2))
    timed(bits, lines, "stage: bits (dicp_compat2_bits)")
    t_c = timed(common, lines, "stage: common pass (dicp_compat2_common)")
    timed(lambda: _lib.call("dicp_compat2_rank", dev, code, _p(d2), _p(P), N, n, 64, _p(rank), _p(s2), _p(seedpos)), lines, "stage: rank (dicp_compat2_rank)")
    timed(lambda: _lib.call("dicp_compat2_seeds", dev, code, _p(pairs), _p(P), _p(adj), _p(seedpos), N, n, 64, 16, _p(mem), _p(poses)), lines,
          "stage: seed rows + fit (dicp_compat2_seeds)")
    word_pairs = float(N) * n * n * W
    rate = word_pairs / (t_c * 1e-3)
    lines.append("    common pass: %.3g word pairs, %.3g word pairs / s = %.1f %% of the vector issue rate at %d operations per pair (%.3g wave instructions / s)"
                 % (word_pairs, rate, 100.0 * rate * OPS_PER_WORD_PAIR / 64 / WAVE_ISSUE_PER_S, OPS_PER_WORD_PAIR, WAVE_ISSUE_PER_S))
    print(lines[-1], flush=True)


def angle(C, C_true):
    R = C.double().cpu() @ C_true.T
    ax = torch.stack((R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]), dim=1) / 2
    return torch.atan2(ax.norm(dim=1), (R.diagonal(dim1=1, dim2=2).sum(dim=1) - 1) / 2)


def found(name, T, inl, truth, C, lines):
    err = angle(T[:, :3, :3], C)
    share = (inl & truth).sum(dim=1).double() / truth.sum(dim=1).clamp(min=1).double()
    lines.append("        %-44s clouds within 0.02 rad %2d / %d, median rotation error %.3g rad, worst %.3g rad, true inliers found %.3f (mean share), inliers %.1f (mean)"
                 % (name, int((err < 0.02).sum()), N, float(err.median()), float(err.max()), float(share.mean()), float(inl.sum(dim=1).double().mean())))
    print(lines[-1], flush=True)


def step(n, dtype, out):
    dt = {"float32": torch.float32, "float64": torch.float64}[dtype]
    lines = ["%d clouds x %d matches, %s, 10 %% inliers" % (N, n, dtype)]
    print(lines[-1], flush=True)
    x, y, idx, truth, C = make(N, n, 0.1, dt)
    stage_times(x, y, idx, lines)
    t2 = timed(lambda: M.prune_correspondences(x, y, idx, THR, n // 16, order=2), lines, "prune_correspondences, order 2")
    t1 = timed(lambda: M.prune_correspondences(x, y, idx, THR, n // 16, iterations=10), lines, "prune_correspondences, order 1, iterations 10")
    lines.append("    order 2 / order 1: %.2f x the time" % (t2 / t1))
    k2, _ = M.prune_correspondences(x, y, idx, THR, n // 16, order=2)
    k1, _ = M.prune_correspondences(x, y, idx, THR, n // 16, iterations=10)
    lines.append("    kept that are true: order 2 %.3f, order 1 %.3f (keep = n / 16)"
                 % (float(((k2 >= 0) & truth).sum()) / float((k2 >= 0).sum()), float(((k1 >= 0) & truth).sum()) / float((k1 >= 0).sum())))
    print("\n".join(lines[-2:]), flush=True)
    timed(lambda: M.consensus_correspondences(x, y, idx, THR, inlier_threshold=3 * THR, seeds=64), lines, "consensus_correspondences, seeds 64")
    timed(lambda: M.ransac_correspondences(x, y, idx, 3 * THR, hypotheses=1024, seed=1), lines, "ransac_correspondences, H 1024")
    timed(lambda: M.ransac_correspondences(x, y, idx, 3 * THR, hypotheses=4096, seed=1), lines, "ransac_correspondences, H 4096")
    for ratio in (0.1, 0.05, 0.01):
        x, y, idx, truth, C = make(N, n, ratio, dt, seed=1)
        lines.append("    %g %% inliers (%.1f true matches per cloud):" % (100 * ratio, float(truth.sum(dim=1).double().mean())))
        print(lines[-1], flush=True)
        found("consensus_correspondences, seeds 64", *M.consensus_correspondences(x, y, idx, THR, inlier_threshold=3 * THR, seeds=64), truth, C, lines)
        for H in (1024, 4096):
            found("ransac_correspondences, H %d" % H, *M.ransac_correspondences(x, y, idx, 3 * THR, hypotheses=H, seed=1), truth, C, lines)
    torch.cuda.synchronize()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_compat2_bench.txt"))
    ap.add_argument("--quick", action="store_true", help="float32, 2048 and 4096 matches only")
    ap.add_argument("--step", nargs=2, metavar=("MATCHES", "DTYPE"), help="run one step (what the driver starts)")
    a = ap.parse_args()
    if a.step:
        step(int(a.step[0]), a.step[1], a.out)
        return 0
    head = ["# second-order compatibility and seeded consensus on %s: %d clouds, threshold %g, inlier threshold %g, medians of 5" % (torch.cuda.get_device_name(0), N, THR, 3 * THR),
            "# keep = n / 16, seeds 64, members 16, refine 1; the stages are the library calls on the packed pairs; every other line is the public function",
            "# (dicp_select_rows, the outputs' gathers and the final fit included)"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(head) + "\n")
    part = a.out + ".part"
    for dtype in (("float32",) if a.quick else ("float32", "float64")):
        for n in ((2048, 4096) if a.quick else (2048, 4096, 16384)):
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(n), dtype, "--out", part], timeout=STEP_LIMIT_S).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:                                         # nothing more is started on the GPU after a failure
                with open(a.out, "a") as f:
                    f.write("step %d %s ended with status %d: the run stops here\n" % (n, dtype, rc))
                return rc
            with open(part) as g, open(a.out, "a") as f:
                f.write(g.read())
            os.remove(part)
    return 0


if __name__ == "__main__":
    sys.exit(main())
