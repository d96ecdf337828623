"""Times ransac_correspondences stage by stage on one GPU, beside the torch composition a user would write, and writes
profiles/r26_ransac_bench.txt.  Medians of 5 (every sample is printed), 32 clouds x 16384 pairs, H in {1024, 4096}, inlier ratio
0.1 / 0.3 / 0.5, float32 and float64, refine 0 and 1.

    python scripts/ransac_bench.py [--out profiles/r26_ransac_bench.txt] [--quick]
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
from dicp_amd.filter import _Select  # noqa: E402

REPS = 5
VALU_PER_PAIR = 17          # 9 + 3 fma, 3 subtractions, 1 compare, 1 conditional add per (hypothesis, pair), as the source writes them
WAVE_ISSUE_PER_S = 256 * 4 * 2.4e9 / 2      # MI355X: 256 CUs x 4 SIMDs, a wave64 v_fma_f32 issues in 2 cycles, 2.4 GHz


def make(N, n, ratio, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((N, n, 3), generator=g, dtype=torch.float64) * 2 - 1
    ang = 0.7
    C = torch.tensor([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]], dtype=torch.float64)
    y = x @ C.T + torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64) + 0.005 * torch.randn((N, n, 3), generator=g, dtype=torch.float64)
    out = torch.rand((N, n), generator=g) >= ratio
    y[out] = torch.rand((int(out.sum()), 3), generator=g, dtype=torch.float64) * 4 - 2
    idx = torch.arange(n).repeat(N, 1)
    return x.to(dtype).cuda(), y.to(dtype).cuda(), idx.cuda()


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
    lines.append("    %-34s median %9.3f ms   samples %s" % (label, med, " ".join("%.3f" % v for v in ms)))
    print(lines[-1], flush=True)
    return med


def torch_composition(x, y, idx, thr, H, chunk):
    """what a user would write: random triples, batched SVD Kabsch, residuals chunked over H, counts, argmax"""
    N, n, _ = x.shape
    yg = torch.gather(y, 1, idx[..., None].expand(N, n, 3))
    tri = torch.randint(0, n, (N, H, 3), device=x.device)
    px = torch.gather(x[:, None].expand(N, H, n, 3), 2, tri[..., None].expand(N, H, 3, 3))
    py = torch.gather(yg[:, None].expand(N, H, n, 3), 2, tri[..., None].expand(N, H, 3, 3))
    mx, my = px.mean(dim=2, keepdim=True), py.mean(dim=2, keepdim=True)
    W = (py - my).transpose(2, 3) @ (px - mx)
    U, _, Vt = torch.linalg.svd(W)
    d = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
    D = torch.diag_embed(torch.stack((torch.ones_like(d), torch.ones_like(d), d), dim=-1))
    C = U @ D @ Vt
    r = my[:, :, 0] - (C @ mx.transpose(2, 3))[..., 0]
    counts = torch.empty((N, H), dtype=torch.int64, device=x.device)
    for h0 in range(0, H, chunk):
        q = torch.einsum("bhac,bnc->bhna", C[:, h0:h0 + chunk], x) + r[:, h0:h0 + chunk, None, :]
        counts[:, h0:h0 + chunk] = (((q - yg[:, None]) ** 2).sum(-1) <= thr * thr).sum(-1)
    return counts.argmax(dim=1), C, r


def torch_score_only(x, yg, C, r, thr, chunk):
    N, H = C.shape[0], C.shape[1]
    counts = torch.empty((N, H), dtype=torch.int64, device=x.device)
    for h0 in range(0, H, chunk):
        q = torch.einsum("bhac,bnc->bhna", C[:, h0:h0 + chunk], x) + r[:, h0:h0 + chunk, None, :]
        counts[:, h0:h0 + chunk] = (((q - yg[:, None]) ** 2).sum(-1) <= thr * thr).sum(-1)
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_ransac_bench.txt"))
    ap.add_argument("--quick", action="store_true", help="float32, H = 1024, ratio 0.3 only")
    a = ap.parse_args()
    N, n, thr = 32, 16384, 0.02
    lines = ["# ransac_correspondences on %s: %d clouds x %d pairs, threshold %g, medians of %d" % (torch.cuda.get_device_name(0), N, n, thr, REPS),
             "# score: %d vector instructions per (hypothesis, pair) as the source writes them; issue peak %.4g wave-instructions/s" % (VALU_PER_PAIR, WAVE_ISSUE_PER_S)]
    print("\n".join(lines), flush=True)
    table = []
    for dtype in ((torch.float32,) if a.quick else (torch.float32, torch.float64)):
        for H in ((1024,) if a.quick else (1024, 4096)):
            for ratio in ((0.3,) if a.quick else (0.1, 0.3, 0.5)):
                x, y, idx = make(N, n, ratio, dtype)
                code, dev = _DT[dtype], x.device
                lines.append("%s H %d inlier ratio %.1f" % (str(dtype).split(".")[1], H, ratio))
                print(lines[-1], flush=True)
                idx32 = M._idx32(idx, n)
                st = {}

                def pack():
                    yg = torch.gather(y, 1, idx32.clamp(min=0, max=n - 1).long()[..., None].expand(N, n, 3))
                    live = (idx32 >= 0) & torch.isfinite(x).all(dim=-1) & torch.isfinite(yg).all(dim=-1)
                    st["pairs"], st["P"], _ = _Select.apply(torch.cat((x, yg), dim=-1).contiguous(), live.contiguous(), None, True)
                t_pack = timed(pack, lines, "pack (gather, mask, select_rows)")
                poses = torch.empty((N, H, 12), dtype=dtype, device=dev)
                samples = torch.empty((N, H, 3), dtype=torch.int32, device=dev)
                counts = torch.empty((N, H), dtype=torch.int32, device=dev)
                best = torch.empty((N,), dtype=torch.int32, device=dev)
                bc = torch.empty((N,), dtype=torch.int32, device=dev)
                pb = torch.empty((N, 12), dtype=dtype, device=dev)
                t_hyp = timed(lambda: _lib.call("dicp_ransac_hypotheses", dev, code, _p(st["pairs"]), _p(st["P"]), N, n, H, 7, _p(poses), _p(samples)), lines,
                              "hypotheses")

                def score():
                    _lib.call("dicp_zero", dev, _p(counts), counts.numel() * 4)
                    _lib.call("dicp_ransac_score", dev, code, _p(st["pairs"]), _p(st["P"]), _p(poses), N, n, H, thr, _p(counts))
                t_score = timed(score, lines, "score (zero + kernel)")
                t_best = timed(lambda: _lib.call("dicp_ransac_best", dev, code, _p(counts), _p(poses), _p(st["P"]), N, H, _p(best), _p(bc), _p(pb)), lines, "best")
                thr2 = torch.full((), thr * thr, dtype=dtype, device=dev)
                t_res = timed(lambda: M._residuals(x, y, idx32, None, pb) <= thr2, lines, "residual round (I_0)")
                inl = M._residuals(x, y, idx32, None, pb) <= thr2
                minus = torch.full_like(idx, -1)

                def refit():
                    pj = M._pose12(M._align(x, y, torch.where(inl, idx, minus), None, None))
                    return M._residuals(x, y, idx32, None, pj) <= thr2
                t_ref = timed(refit, lines, "refine round (fit + residuals)")
                t_fit = timed(lambda: M._align(x, y, torch.where(inl, idx, minus), None, None), lines, "final fit")
                t0 = timed(lambda: M.ransac_correspondences(x, y, idx, thr, hypotheses=H, seed=7, refine=0), lines, "whole call, refine 0")
                t1 = timed(lambda: M.ransac_correspondences(x, y, idx, thr, hypotheses=H, seed=7, refine=1), lines, "whole call, refine 1")
                chunk = 64 if dtype == torch.float32 else 32
                t_torch = timed(lambda: torch_composition(x, y, idx, thr, H, chunk), lines, "torch composition (chunk %d)" % chunk)
                _, C, r = torch_composition(x, y, idx, thr, H, chunk)
                yg = torch.gather(y, 1, idx[..., None].expand(N, n, 3))
                t_tscore = timed(lambda: torch_score_only(x, yg, C, r, thr, chunk), lines, "torch residuals + counts only")
                Psum = float(st["P"].sum())
                frac = Psum * H * VALU_PER_PAIR / 64.0 / (t_score * 1e-3) / WAVE_ISSUE_PER_S
                lines.append("    score: %.3g (hypothesis, pair) per second, %.1f %% of the f32 vector issue rate at %d instructions each; found %d of %d expected inliers in cloud 0"
                             % (Psum * H / (t_score * 1e-3), 100 * frac, VALU_PER_PAIR, int(bc[0]), int(round(ratio * n))))
                print(lines[-1], flush=True)
                table.append((str(dtype).split(".")[1], H, ratio, t_pack, t_hyp, t_score, t_best, t_res, t_ref, t_fit, t0, t1, t_torch, t_tscore, 100 * frac))
                del x, y, idx, poses, samples, C, r, yg
                torch.cuda.empty_cache()
    lines.append("")
    lines.append("| dtype | H | inliers | pack | hypotheses | score | best | residuals | refine round | final fit | call R=0 | call R=1 | torch | torch score | score %issue |")
    lines.append("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for t in table:
        lines.append("| %s | %d | %.1f | " % t[:3] + " | ".join("%.3f" % v for v in t[3:14]) + " | %.1f |" % t[14])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-len(table) - 2:]))


if __name__ == "__main__":
    main()
