"""Times gnc_correspondences part by part on one GPU, beside ransac_correspondences at H = 1024 and 4096 and the torch composition a user
would write (a loop of residuals, weights and a weighted batched torch.linalg.svd Kabsch, with an .item() for the stop test), with the
rotation error of each, and writes profiles/r32_gnc_bench.txt.  Medians of 5 (every sample is printed): 32 and 256 clouds x 2048 and 16384
pairs, inlier ratio 0.3 / 0.5, float32 and float64, both losses.  A last block times the launch on clouds of 64 pairs: the floor of a round
(lane 0's fit, the reduction and the barriers), beside which the per-pair slope of the large clouds stands.

    python scripts/gnc_bench.py [--out profiles/r32_gnc_bench.txt] [--quick]
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
from dicp_amd import register as M  # noqa: E402
from dicp_amd._ops import _DT, _p  # noqa: E402

REPS = 5
ANGLE = 0.7
C_TRUE = np.array([[np.cos(ANGLE), -np.sin(ANGLE), 0], [np.sin(ANGLE), np.cos(ANGLE), 0], [0, 0, 1.0]])


def make(N, n, ratio, dtype, seed=0):
    """scripts/ransac_bench.py's clouds: x in [-1, 1]^3, y = C x + r + 0.005 noise for the inliers, uniform in [-2, 2]^3 for the rest"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((N, n, 3), generator=g, dtype=torch.float64) * 2 - 1
    y = x @ torch.tensor(C_TRUE).T + torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64) + 0.005 * torch.randn((N, n, 3), generator=g, dtype=torch.float64)
    out = torch.rand((N, n), generator=g) >= ratio
    y[out] = torch.rand((int(out.sum()), 3), generator=g, dtype=torch.float64) * 4 - 2
    idx = torch.arange(n).repeat(N, 1)
    return x.to(dtype).cuda(), y.to(dtype).cuda(), idx.cuda()


def rotation_errors(T):
    """(N, 4, 4) or a list of (C (N, 3, 3)) -> (median, max) angle to the truth over the clouds, radians"""
    C = T[:, :3, :3].double().cpu().numpy()
    tr = np.einsum("bij,ij->b", C, C_TRUE)
    err = np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0))
    return float(np.median(err)), float(err.max())


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
    lines.append("    %-38s median %9.3f ms   samples %s" % (label, med, " ".join("%.3f" % v for v in ms)))
    print(lines[-1], flush=True)
    return med


def weighted_kabsch(x, yg, w):
    S0 = w.sum(dim=1, keepdim=True).clamp(min=1e-30)[..., None]
    mx, my = (w[..., None] * x).sum(dim=1, keepdim=True) / S0, (w[..., None] * yg).sum(dim=1, keepdim=True) / S0
    W = ((yg - my) * w[..., None]).transpose(1, 2) @ (x - mx)
    U, _, Vt = torch.linalg.svd(W)
    d = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
    D = torch.diag_embed(torch.stack((torch.ones_like(d), torch.ones_like(d), d), dim=-1))
    C = U @ D @ Vt
    return C, my[:, 0] - (C @ mx.transpose(1, 2))[..., 0]


def torch_gnc(x, yg, thr, loss, growth=1.4, iterations=128):
    """what a user would write: the schedule of gnc_correspondences in batched torch ops, a cloud frozen once it meets its stopping rule"""
    def resid(C, r):
        return ((x @ C.transpose(1, 2) + r[:, None] - yg) ** 2).sum(-1)
    c2 = thr * thr
    w = torch.ones(x.shape[:2], dtype=x.dtype, device=x.device)
    C, r = weighted_kabsch(x, yg, w)
    d = resid(C, r)
    dmax = d.amax(dim=1, keepdim=True)
    mu = c2 / (2 * dmax - c2) if loss == "tls" else (2 * dmax / c2).clamp(min=1.0)
    active = (2 * dmax > c2) if loss == "tls" else torch.ones_like(dmax, dtype=torch.bool)
    rounds = 0
    for _ in range(iterations):
        if loss == "tls":
            lo, hi = mu / (mu + 1) * c2, (mu + 1) / mu * c2
            band = (d > lo) & (d < hi)
            wn = torch.where(d <= lo, 1.0, torch.where(band, torch.sqrt(c2 * mu * (mu + 1) / d) - mu, 0.0)).to(x.dtype)
            done = band.sum(dim=1, keepdim=True) == 0
        else:
            wn = (mu * c2 / (d + mu * c2)) ** 2
            done = mu <= 1.0
        w = torch.where(active, wn, w)
        Cn, rn = weighted_kabsch(x, yg, w)
        C, r = torch.where(active[..., None], Cn, C), torch.where(active, rn, r)
        d = resid(C, r)
        rounds += 1
        active = active & ~done
        if not bool(active.any().item()):
            break
        mu = torch.where(active, mu * growth if loss == "tls" else (mu / growth).clamp(min=1.0), mu)
    return C, rounds


def launch_only(st, N, n, dtype, loss, thr):
    dev = st["pairs"].device
    wp = torch.empty((N, n), dtype=dtype, device=dev)
    rounds = torch.empty((N,), dtype=torch.int32, device=dev)
    status = torch.empty((N,), dtype=torch.int32, device=dev)
    mu = torch.empty((N,), dtype=torch.float64, device=dev)
    pose = torch.empty((N, 12), dtype=dtype, device=dev)

    def fn():
        _lib.call("dicp_gnc_fit", dev, _DT[dtype], _p(st["pairs"]), _p(st["P"]), None, N, n, M.GNC_LOSSES[loss], thr, 1.4, 128, _p(wp), _p(rounds), _p(status),
                  _p(mu), _p(pose), None)
    return fn, rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_gnc_bench.txt"))
    ap.add_argument("--quick", action="store_true", help="float32, 32 clouds x 2048 pairs, ratio 0.5 only")
    a = ap.parse_args()
    thr = 0.02
    lines = ["# gnc_correspondences on %s: threshold %g, growth 1.4, iterations 128, medians of %d; rotation errors: median / max over the clouds, radians"
             % (torch.cuda.get_device_name(0), thr, REPS)]
    print(lines[0], flush=True)
    table = []
    shapes = ((32, 2048),) if a.quick else ((32, 2048), (32, 16384), (256, 2048), (256, 16384))
    for dtype in ((torch.float32,) if a.quick else (torch.float32, torch.float64)):
        for N, n in shapes:
            for ratio in ((0.5,) if a.quick else (0.3, 0.5)):
                x, y, idx = make(N, n, ratio, dtype)
                name = str(dtype).split(".")[1]
                lines.append("%s %d clouds x %d pairs, inlier ratio %.1f" % (name, N, n, ratio))
                print(lines[-1], flush=True)
                st = {}

                def pack():
                    pk = M._live_pairs(x, y, idx, None)
                    st["pairs"], st["P"] = pk.pairs, pk.P
                t_pack = timed(pack, lines, "pack (gather, mask, select_rows)")
                ransac = {}
                for H in (1024, 4096):
                    ransac[H] = timed(lambda: M.ransac_correspondences(x, y, idx, thr, hypotheses=H, seed=7), lines, "ransac_correspondences H %d" % H)
                    ransac[H, "err"] = rotation_errors(M.ransac_correspondences(x, y, idx, thr, hypotheses=H, seed=7)[0])
                    lines.append("        rotation error %.3e / %.3e" % ransac[H, "err"])
                yg = torch.gather(y, 1, idx[..., None].expand(N, n, 3))
                for loss in ("tls", "gm"):
                    lines.append("  loss %s" % loss)
                    fn, rounds = launch_only(st, N, n, dtype, loss, thr)
                    t_launch = timed(fn, lines, "dicp_gnc_fit (one launch)")
                    rmean, rmax = float(rounds.float().mean()), int(rounds.max())
                    T, w = M.gnc_correspondences(x, y, idx, thr, loss=loss)
                    minus = torch.full_like(idx, -1)
                    t_fit = timed(lambda: M._align(x, y, torch.where(w > 0, idx, minus), w, None), lines, "final fit")
                    t_call = timed(lambda: M.gnc_correspondences(x, y, idx, thr, loss=loss), lines, "whole call")
                    err = rotation_errors(T)
                    t_torch = timed(lambda: torch_gnc(x, yg, thr, loss), lines, "torch composition")
                    Ct, trounds = torch_gnc(x, yg, thr, loss)
                    terr = rotation_errors(Ct)
                    lines.append("        rounds mean %.1f max %d (torch loop: %d); %.2f us per round of the slowest cloud; rotation error GNC %.3e / %.3e, torch %.3e / %.3e"
                                 % (rmean, rmax, trounds, 1e3 * t_launch / max(rmax, 1), err[0], err[1], terr[0], terr[1]))
                    print(lines[-1], flush=True)
                    table.append((name, N, n, ratio, loss, t_pack, t_launch, rmean, t_fit, t_call, t_torch, ransac[1024], ransac[4096], err[1], terr[1],
                                  ransac[1024, "err"][1], ransac[4096, "err"][1]))
                del x, y, idx, yg
                torch.cuda.empty_cache()
    # the floor of a round: clouds of 64 pairs, one pair in each lane of the first wave, nothing to walk
    lines.append("the floor of a round: 256 clouds x 64 pairs, float32, inlier ratio 0.5 (lane 0's fit, the reduction, the barriers)")
    print(lines[-1], flush=True)
    x, y, idx = make(256, 64, 0.5, torch.float32)
    st = {}
    pk = M._live_pairs(x, y, idx, None)
    st["pairs"], st["P"] = pk.pairs, pk.P
    for loss in ("tls", "gm"):
        fn, rounds = launch_only(st, 256, 64, torch.float32, loss, thr)
        t = timed(fn, lines, "dicp_gnc_fit %s" % loss)
        lines.append("        rounds mean %.1f max %d: %.2f us per round of the slowest cloud" % (float(rounds.float().mean()), int(rounds.max()), 1e3 * t / max(int(rounds.max()), 1)))
        print(lines[-1], flush=True)
    lines.append("")
    lines.append("| dtype | clouds | pairs | inliers | loss | pack | GNC launch | rounds | final fit | whole call | torch | RANSAC 1024 | RANSAC 4096 | "
                 "err GNC | err torch | err R1024 | err R4096 |")
    lines.append("|" + "---|" * 17)
    for t in table:
        lines.append("| %s | %d | %d | %.1f | %s | %.3f | %.3f | %.1f | %.3f | %.3f | %.3f | %.3f | %.3f | %.1e | %.1e | %.1e | %.1e |" % t)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-len(table) - 2:]))


if __name__ == "__main__":
    main()
