"""Times correspondence_compatibility / prune_correspondences on one GPU, beside the torch composition a user would write, and writes
profiles/r29_compat_bench.txt.  Medians of 5 (every sample is printed): 32 clouds x {2048, 4096, 16384} matches, float32 and float64,
iterations 0 and 10; then ransac_correspondences at H = 4096 on every match against H = 256 on the pruned matches, on the 10 % line of
scripts/ransac_bench.py's generator.

    python scripts/compat_bench.py [--out profiles/r29_compat_bench.txt] [--quick]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dicp_amd import _lib  # noqa: E402
from dicp_amd import match as M  # noqa: E402
from dicp_amd._pairs import _live_pairs  # noqa: E402
from dicp_amd._ops import _DT, _p  # noqa: E402

REPS = 5
OPS_PER_PAIR = 20           # 6 subtractions, 6 fma, 2 square roots, 1 subtraction, 4 compares, 1 conditional add per (p, q), as the source writes them
WAVE_ISSUE_PER_S = 256 * 4 * 2.4e9 / 2      # MI355X: 256 CUs x 4 SIMDs, a wave64 v_fma_f32 issues in 2 cycles, 2.4 GHz


def make(N, n, ratio, dtype, seed=0):
    """scripts/ransac_bench.py's generator, with the truth"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((N, n, 3), generator=g, dtype=torch.float64) * 2 - 1
    ang = 0.7
    C = torch.tensor([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]], dtype=torch.float64)
    y = x @ C.T + torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64) + 0.005 * torch.randn((N, n, 3), generator=g, dtype=torch.float64)
    out = torch.rand((N, n), generator=g) >= ratio
    y[out] = torch.rand((int(out.sum()), 3), generator=g, dtype=torch.float64) * 4 - 2
    idx = torch.arange(n).repeat(N, 1)
    return x.to(dtype).cuda(), y.to(dtype).cuda(), idx.cuda(), (~out).cuda(), C


def timed(fn, lines, label):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    med = statistics.median(ms)
    lines.append("    %-44s median %10.3f ms   samples %s" % (label, med, " ".join("%.3f" % v for v in ms)))
    print(lines[-1], flush=True)
    return med


def torch_composition(x, y, idx, thr, iterations):
    """what a user writes without the kernels, per cloud: two (n, n) cdist matrices, the mask, then M @ v"""
    N, n, _ = x.shape
    yg = torch.gather(y, 1, idx[..., None].expand(N, n, 3))
    score = torch.empty((N, n), dtype=x.dtype, device=x.device)
    degree = torch.empty((N, n), dtype=torch.int64, device=x.device)
    for b in range(N):
        Mb = (torch.cdist(x[b], x[b]) - torch.cdist(yg[b], yg[b])).abs() <= thr
        degree[b] = Mb.sum(dim=1) - 1
        Mf = Mb.to(x.dtype)
        v = torch.ones((n,), dtype=x.dtype, device=x.device)
        for _ in range(iterations):
            w = Mf @ v
            v = w / w.max()
        score[b] = v
    return score, degree


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_compat_bench.txt"))
    ap.add_argument("--quick", action="store_true", help="float32, 2048 and 4096 matches only")
    a = ap.parse_args()
    N, thr = 32, 0.02
    lines = ["# correspondence_compatibility on %s: %d clouds, threshold %g, inlier ratio 0.1, medians of %d" % (torch.cuda.get_device_name(0), N, thr, REPS),
             "# pass: %d operations per (p, q) as the source writes them (each correctly rounded square root expands into a v_sqrt and its correction);"
             " issue peak %.4g wave-instructions/s" % (OPS_PER_PAIR, WAVE_ISSUE_PER_S)]
    print("\n".join(lines), flush=True)
    table = []
    for dtype in ((torch.float32,) if a.quick else (torch.float32, torch.float64)):
        for n in ((2048, 4096) if a.quick else (2048, 4096, 16384)):
            x, y, idx, truth, _ = make(N, n, 0.1, dtype)
            code, dev = _DT[dtype], x.device
            name = str(dtype).split(".")[1]
            lines.append("%s n %d" % (name, n))
            print(lines[-1], flush=True)
            pk = _live_pairs(x, y, idx, None)
            live, pairs, P = pk.live, pk.pairs, pk.P
            w = torch.empty((2, N, n), dtype=dtype, device=dev)
            sp = torch.empty((N, n), dtype=dtype, device=dev)
            dp = torch.empty((N, n), dtype=torch.int32, device=dev)
            rank = torch.empty((N, n), dtype=torch.int32, device=dev)
            t_pack = timed(lambda: _live_pairs(x, y, idx, None), lines, "pack (gather, mask, select_rows)")

            def scores(it):
                wmax = torch.zeros((max(it, 1), N), dtype=torch.int32 if dtype == torch.float32 else torch.int64, device=dev)
                _lib.call("dicp_compat_scores", dev, code, _p(pairs), _p(P), N, n, it, thr, 0.0, _p(w), _p(wmax), _p(sp), _p(dp))
            t_s0 = timed(lambda: scores(0), lines, "dicp_compat_scores, iterations 0 (1 pass)")
            t_s10 = timed(lambda: scores(10), lines, "dicp_compat_scores, iterations 10 (10 passes)")
            t_pass = (t_s10 - t_s0) / 9.0
            t_rank = timed(lambda: _lib.call("dicp_compat_rank", dev, code, _p(sp), _p(P), N, n, _p(rank)), lines, "dicp_compat_rank")
            t_c0 = timed(lambda: M.correspondence_compatibility(x, y, idx, thr, iterations=0), lines, "correspondence_compatibility, iterations 0")
            t_c10 = timed(lambda: M.correspondence_compatibility(x, y, idx, thr, iterations=10), lines, "correspondence_compatibility, iterations 10")
            t_p10 = timed(lambda: M.prune_correspondences(x, y, idx, thr, n // 16, iterations=10), lines, "prune_correspondences, iterations 10")
            t_t0 = timed(lambda: torch_composition(x, y, idx, thr, 0), lines, "torch composition, iterations 0")
            t_t10 = timed(lambda: torch_composition(x, y, idx, thr, 10), lines, "torch composition, iterations 10")
            pairs_per_pass = float((P.double() ** 2).sum())
            frac = pairs_per_pass * OPS_PER_PAIR / 64.0 / (t_pass * 1e-3) / WAVE_ISSUE_PER_S
            score, degree = M.correspondence_compatibility(x, y, idx, thr, iterations=10)
            ts, td = torch_composition(x, y, idx, thr, 10)
            kept, _ = M.prune_correspondences(x, y, idx, thr, n // 16, iterations=10)
            lines.append("    pass: %.3f ms, %.3g (p, q) per second, %.1f %% of the f32 vector issue rate at %d operations each; degree differs from torch's on %d of %d rows,"
                         " max |score - torch's| %.3g; %d of the %d kept per cloud are true (mean)"
                         % (t_pass, pairs_per_pass / (t_pass * 1e-3), 100 * frac, OPS_PER_PAIR, int((degree != td).sum()), N * n, float((score - ts).abs().max()),
                            int(((kept >= 0) & truth).sum()) // N, n // 16))
            print(lines[-1], flush=True)
            table.append((name, n, t_pack, t_s0, t_s10, t_pass, t_rank, t_c0, t_c10, t_p10, t_t0, t_t10, 100 * frac))
            del x, y, idx, pairs, w, sp, dp, rank, ts, td
            torch.cuda.empty_cache()
    lines.append("")
    lines.append("| dtype | n | pack | scores it=0 | scores it=10 | per pass | rank | call it=0 | call it=10 | prune it=10 | torch it=0 | torch it=10 | pass %issue |")
    lines.append("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for t in table:
        lines.append("| %s | %d | " % t[:2] + " | ".join("%.3f" % v for v in t[2:12]) + " | %.1f |" % t[12])
    # ------------------------------------------------------------------ RANSAC on every match against RANSAC on the pruned matches
    lines.append("")
    lines.append("ransac_correspondences, 32 x 16384 matches at 10 %% inliers (threshold %g, refine 1, seed 7): every match at H = 4096 against the pruned matches at H = 256" % thr)
    n, keep = 16384, 1024
    for dtype in ((torch.float32,) if a.quick else (torch.float32, torch.float64)):
        x, y, idx, truth, C = make(N, n, 0.1, dtype)
        name = str(dtype).split(".")[1]
        lines.append("%s" % name)
        t_plain = timed(lambda: M.ransac_correspondences(x, y, idx, thr, hypotheses=4096, seed=7), lines, "ransac H = 4096, every match")

        def pruned():
            kept, _ = M.prune_correspondences(x, y, idx, thr, keep, iterations=10)
            return M.ransac_correspondences(x, y, kept, thr, hypotheses=256, seed=7)
        t_pruned = timed(pruned, lines, "prune (keep %d) + ransac H = 256" % keep)
        kept, _ = M.prune_correspondences(x, y, idx, thr, keep, iterations=10)
        t_r256 = timed(lambda: M.ransac_correspondences(x, y, kept, thr, hypotheses=256, seed=7), lines, "ransac H = 256 on the pruned matches alone")
        for label, (T, inl), among in (("every match, H = 4096", M.ransac_correspondences(x, y, idx, thr, hypotheses=4096, seed=7), truth),
                                       ("pruned, H = 256", pruned(), truth & (kept >= 0))):
            R = T[:, :3, :3].double().cpu() @ C.T
            err = torch.acos(((R.diagonal(dim1=1, dim2=2).sum(-1) - 1) / 2).clamp(-1, 1))
            lines.append("    %-24s inliers found per cloud: min %d, median %d, max %d of %d true ones among the matches given (mean); rotation error median %.3g, max %.3g rad"
                         % (label, int(inl.sum(1).min()), int(inl.sum(1).median()), int(inl.sum(1).max()), int(among.sum()) // N, float(err.median()), float(err.max())))
            print(lines[-1], flush=True)
        lines.append("    kept matches that are true: %d of %d per cloud (mean)" % (int(((kept >= 0) & truth).sum()) // N, keep))
        lines.append("    times: %.3f ms against %.3f ms (%.3f ms of it RANSAC)" % (t_plain, t_pruned, t_r256))
        print("\n".join(lines[-2:]), flush=True)
        del x, y, idx
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
