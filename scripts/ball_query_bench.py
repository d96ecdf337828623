"""ball_query at B = 256 x 16384 queries against 16384 rows (float32), at radii whose mean count is about 1, 8 and 32, with k = 8 and 32:
the whole call forward and forward + backward, the grid build on its own, the mean rows scanned per query -- and, in the same process on
the same clouds, interleaved call by call, knn_points at the same k (forward, forward + backward, rows walked).  On make_pairs (uniform
volume) and make_scene_pairs (planar) clouds and on a wall perpendicular to x, the slow case of the x-sorted walk.  Every time is the
median of --reps calls after warm-up, each between two HIP events, profiler off.  The radius of a target count is found by bisection on
the counts of the first 4 clouds.  The goal line: the k = 8 forward at mean count ~ 8 against knn_points(k = 8)'s forward of the same run.
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/ball_query_bench.py [--clouds 256] [--points 16384] [--reps 5]
-> profiles/r12_ball_query_bench.txt"""
import argparse
import json
import statistics

import torch

from dicp_amd import _lib
from dicp_amd._ops import _DT, _p, _stream
from dicp_amd.ball import CellGrid, ball_query
from dicp_amd.knn import _Prepared, knn_points
from dicp_amd.synthetic import make_pairs, make_scene_pairs


def make_wall_pairs(N, n, m, seed=0):
    """rows on the plane x = 0 of a 10 x 10 wall, queries within 0.05 of it"""
    g = torch.Generator().manual_seed(seed)
    y = torch.rand((N, m, 3), generator=g) * 10.0
    y[..., 0] = 0.0
    x = torch.rand((N, n, 3), generator=g) * 10.0
    x[..., 0] = (torch.rand((N, n), generator=g) - 0.5) * 0.1
    return x, y


def timed(fns, reps, warmup=2):
    """medians (ms) of reps calls of every function, the functions taking turns, each call between two HIP events"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [statistics.median(t) for t in ts]


def mean_count(x, y, r):
    return ball_query(x[:4], y[:4], r, k=1, return_counts=True)[2].float().mean().item()


def radius_for(x, y, target):
    lo, hi = 1e-4, 1e2
    for _ in range(30):
        mid = (lo * hi) ** 0.5
        if mean_count(x, y, mid) < target:
            lo = mid
        else:
            hi = mid
    return (lo * hi) ** 0.5


def rows_scanned(x, y, r, k):
    visited = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
    ball_query(x, y, r, k=k, _visited=visited)
    return visited.sum().item() / (x.shape[0] * x.shape[1])


def rows_walked(x, y, k):
    """mean rows visited per query by one knn_points search (the library's diagnostic counters)"""
    N, n, _ = x.shape
    m = y.shape[1]
    px, py = _Prepared(x, None), _Prepared(y, None)
    lib = _lib.load()
    dt = _DT[x.dtype]
    ws_bytes = lib.dicp_knn_points_workspace_bytes(dt, N, n, m, k, 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    d2 = torch.empty((N, n, k), dtype=x.dtype, device=x.device)
    idx = torch.empty((N, n, k), dtype=torch.int64, device=x.device)
    walked = torch.zeros(N, dtype=torch.int64, device=x.device)
    _lib.check(lib.dicp_knn_points(dt, _p(px.tgs4), _p(px.perm), None, n, _p(py.keys), _p(py.tgs4), _p(py.perm), None, m, N, k, _p(d2), _p(idx),
                                   _p(ws), ws_bytes, _p(walked), _stream()), "dicp_knn_points")
    return walked.sum().item() / (N * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="8,32")
    ap.add_argument("--counts", default="1,8,32")
    a = ap.parse_args()
    gens = {"pairs": make_pairs, "scene": make_scene_pairs, "wall": make_wall_pairs}
    goal = []
    for name, gen in gens.items():
        src, tgt = gen(a.clouds, a.points, a.points, seed=1)
        x = src[..., :3].contiguous().cuda()
        y = tgt[..., :3].contiguous().cuda()
        for target in [float(v) for v in a.counts.split(",")]:
            r = radius_for(x, y, target)
            r_d = torch.full((1,), r, dtype=x.dtype, device=x.device)
            for k in [int(v) for v in a.ks.split(",")]:
                xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
                g = torch.randn((a.clouds, a.points, k), device=x.device)

                def ball_fb():
                    xg.grad = yg.grad = None
                    d2 = ball_query(xg, yg, r, k=k)[0]
                    (torch.where(torch.isfinite(d2), d2, torch.zeros_like(d2)) * g).sum().backward()

                def knn_fb():
                    xg.grad = yg.grad = None
                    (knn_points(xg, yg, k=k)[0] * g).sum().backward()
                fwd, kfwd, fb, kfb, build = timed([lambda: ball_query(x, y, r, k=k), lambda: knn_points(x, y, k=k), ball_fb, knn_fb,
                                                   lambda: CellGrid(y, None, r_d)], a.reps)
                row = {"clouds": name, "B": a.clouds, "n": a.points, "m": a.points, "k": k, "radius": round(r, 5),
                       "mean_count": round(mean_count(x, y, r), 2), "ball_fwd_ms": round(fwd, 3), "ball_fwd_bwd_ms": round(fb, 3),
                       "grid_build_ms": round(build, 3), "rows_scanned_per_query": round(rows_scanned(x, y, r, k), 1),
                       "knn_points_fwd_ms": round(kfwd, 3), "knn_points_fwd_bwd_ms": round(kfb, 3),
                       "knn_rows_walked_per_query": round(rows_walked(x, y, k), 1)}
                print(json.dumps(row), flush=True)
                if k == 8 and target == 8.0:
                    goal.append((name, fwd, kfwd))
    for name, fwd, kfwd in goal:
        print("# goal (k = 8 forward at mean count ~ 8 below knn_points(k = 8) forward) on %s: %s -- %.3f ms against %.3f ms"
              % (name, "met" if fwd < kfwd else "NOT met", fwd, kfwd), flush=True)


if __name__ == "__main__":
    main()
