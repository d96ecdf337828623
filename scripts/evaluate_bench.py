"""evaluate_registration against the composition a user writes without it, in the same run on the same clouds and poses: per pose a
torch transform, ball_query(k=1), a gather of the matched target rows and masked torch reductions for the count, the sum of d2 and the
nine moments -- run H times for H poses, as a user does today.

Configurations: 256 x 16384 source rows against 16384 target rows at H = 1, and 32 clouds at H in {16, 64}; float32 and float64; a
uniform volume and a planar scene; a radius whose ball holds about 1 row and one that holds about 8; poses near the truth and poses far
off (most queries then have an empty cell range); the source rows in voxel order (as voxel_downsample leaves them) and in random order --
the queries are not re-sorted by cell, so the random order is the cost of that.  Every time is the median of --reps calls after a
warm-up, each between two HIP events.  Beside them: the grid build on its own (its share of the H = 1 call), and how far the two forms'
results are apart (the composition's transform rounds differently, so a count can differ at the radius).
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/evaluate_bench.py [--reps 5] -> profiles/r34_evaluate_bench.txt"""
import argparse
import json
import math
import os
import statistics

import torch

from dicp_amd._grid import CellGrid
from dicp_amd.ball import ball_query
from dicp_amd.evaluate import evaluate_registration, information_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def radius_for(layout, m, k):
    """the radius whose ball holds about k of the m rows (unit cube / unit square)"""
    return (3.0 * k / (4.0 * math.pi * m)) ** (1.0 / 3.0) if layout == "uniform" else math.sqrt(k / (math.pi * m))


def rotations(v):
    """(..., 3) axis-angle vectors -> (..., 3, 3) float64"""
    K = torch.zeros(v.shape[:-1] + (3, 3), dtype=torch.float64)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -v[..., 2], v[..., 1], -v[..., 0]
    K[..., 1, 0], K[..., 2, 0], K[..., 2, 1] = v[..., 2], -v[..., 1], v[..., 0]
    return torch.linalg.matrix_exp(K)


def problem(layout, N, n, H, radius, near, order, dtype, seed=1):
    """target (N, n, 3) in the unit cube, source = the target's rows moved back by the true pose, a little noise added, in voxel or in
    random order; poses (N, H, 4, 4): the truth disturbed by about a third of the radius (near) or moved three cube edges away (far)"""
    g = torch.Generator().manual_seed(seed)
    Y = torch.rand((N, n, 3), generator=g, dtype=torch.float64)
    if layout == "planar":
        Y[..., 2] = 0.02 * torch.sin(9.0 * Y[..., 0]) * torch.cos(7.0 * Y[..., 1])
    C = rotations(torch.randn((N, 3), generator=g, dtype=torch.float64) * 0.5)
    r = torch.rand((N, 3), generator=g, dtype=torch.float64) - 0.5
    P = Y + 0.1 * radius * torch.randn((N, n, 3), generator=g, dtype=torch.float64)
    if order == "voxel":
        cell = (P.clamp(0.0, 1.0) * 32).long().clamp(max=31)
        key = (cell[..., 0] * 32 + cell[..., 1]) * 32 + cell[..., 2]
        perm = torch.argsort(key, dim=1, stable=True)
    else:
        perm = torch.argsort(torch.rand((N, n), generator=g), dim=1)
    P = torch.gather(P, 1, perm[..., None].expand(-1, -1, 3))
    X = torch.matmul(P - r[:, None, :], C)                                  # C^T (p - r)
    dC = rotations(torch.randn((N, H, 3), generator=g, dtype=torch.float64) * (radius / 3.0))
    dr = torch.randn((N, H, 3), generator=g, dtype=torch.float64) * (radius / 3.0) + (0.0 if near else 3.0)
    T = torch.zeros((N, H, 4, 4), dtype=torch.float64)
    T[..., :3, :3] = torch.matmul(dC, C[:, None])
    T[..., :3, 3] = torch.matmul(dC, r[:, None, :, None]).squeeze(-1) + dr
    T[..., 3, 3] = 1.0
    return X.to(dtype).cuda(), Y.to(dtype).cuda(), T.to(dtype).cuda()


def composition(X, Y, T, radius):
    """one pose per cloud, T (N, 4, 4) -> count (N,), sse (N,), first moments (N, 3), second moments (N, 3, 3), all float64"""
    q = torch.baddbmm(T[:, None, :3, 3], X, T[:, :3, :3].transpose(1, 2))
    d2, idx = ball_query(q, Y, radius, k=1)
    hit = idx[..., 0] >= 0
    t = torch.gather(Y, 1, idx.clamp(min=0).expand(-1, -1, 3)).double()
    w = hit.double()
    tw = t * w[..., None]
    return hit.sum(1), torch.where(hit, d2[..., 0], torch.zeros_like(d2[..., 0])).double().sum(1), tw.sum(1), torch.einsum("bni,bnj->bij", tw, t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="256x1,32x16,32x64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r34_evaluate_bench.txt"))
    a = ap.parse_args()
    n = a.points
    lines = []

    def emit(row):
        line = row if isinstance(row, str) else json.dumps(row)
        lines.append(line)
        print(line, flush=True)
        with open(a.out, "w") as fh:                        # (every line as soon as it is measured)
            fh.write("\n".join(lines) + "\n")
    emit("# %s: reps %d, %d points per cloud" % (torch.cuda.get_device_name(0), a.reps, n))
    for shape in a.shapes.split(","):
        N, H = (int(v) for v in shape.split("x"))
        for dtype in (torch.float32, torch.float64):
            for layout in ("uniform", "planar"):
                for k in (1, 8):
                    radius = radius_for(layout, n, k)
                    for near in (True, False):
                        for order in ("voxel", "random"):
                            X, Y, T = problem(layout, N, n, H, radius, near, order, dtype)
                            r_d = torch.full((1,), radius, dtype=dtype, device=X.device)
                            t_fused = timed(lambda: evaluate_registration(X, Y, T, radius), a.reps)
                            t_info = timed(lambda: information_matrix(X, Y, T, radius), a.reps)
                            t_grid = timed(lambda: CellGrid(Y, None, r_d), a.reps)
                            t_comp = timed(lambda: [composition(X, Y, T[:, h], radius) for h in range(H)], a.reps)
                            fit, rmse, cnt = evaluate_registration(X, Y, T, radius)
                            ref = [composition(X, Y, T[:, h], radius) for h in range(min(H, 2))]
                            ref_cnt = torch.stack([v[0] for v in ref], dim=1)
                            ref_rmse = torch.stack([torch.sqrt(v[1] / v[0].clamp(min=1)) for v in ref], dim=1)
                            emit({"N": N, "H": H, "n": n, "m": n, "dtype": str(dtype).replace("torch.", ""), "layout": layout, "rows_in_ball": k,
                                  "radius": round(radius, 5), "poses": "near" if near else "far", "source_order": order,
                                  "fitness_mean": round(float(fit.mean().item()), 4),
                                  "fused_ms": round(t_fused, 3), "information_matrix_ms": round(t_info, 3), "grid_build_ms": round(t_grid, 3),
                                  "grid_build_share_of_fused": round(t_grid / t_fused, 3),
                                  "composition_ms": round(t_comp, 3), "composition_over_fused": round(t_comp / t_fused, 2),
                                  "counts_that_differ_from_the_composition": int((cnt[:, :ref_cnt.shape[1]].long() != ref_cnt).sum().item()),
                                  "max_abs_rmse_difference": float("%.3g" % (rmse[:, :ref_rmse.shape[1]] - ref_rmse).abs().max().item())})
                            del X, Y, T
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
