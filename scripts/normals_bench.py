"""estimate_normals at B = 256 x 16384: forward and forward + backward per k and per method (the x-sorted walk and the cell grid, taking turns
in the same run), on make_pairs targets (uniform volume), on make_scene_pairs targets (planar) and on a wall perpendicular to x (the sorted
walk's slow case), with the mean number of rows a query visits -- the walk's counter, and the grid scan's.  --downsampled adds the pipeline
case: voxel_downsample of 256 x 131072 raw clouds, then the normals of the centroids with rows=.  Every time is the median of --reps calls,
each between two HIP events, after warm-up.
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/normals_bench.py [--method walk,grid] [--clouds 256] [--points 16384] [--reps 10]
-> profiles/r07_normals_bench.txt (walk only), profiles/r14_normals_grid_bench.txt"""
import argparse
import json
import os
import statistics
import sys

import torch

from dicp_amd import _lib
from dicp_amd._ops import _DT, _p, _stream
from dicp_amd.normals import estimate_normals
from dicp_amd.synthetic import make_pairs, make_scene_pairs


def make_wall_pairs(N, n, m, seed=0, dtype=torch.float32):
    """(None, rows on the plane x = 0 of a 10 x 10 wall)"""
    g = torch.Generator().manual_seed(seed)
    y = torch.rand((N, m, 3), generator=g, dtype=torch.float64) * 10.0
    y[..., 0] = 0.0
    return None, y.to(dtype)


def rows_walked(x, k, rows=None):
    """mean rows visited per query by one forward of the walk (the library's diagnostic counters)"""
    N, m, c = x.shape
    lib = _lib.load()
    dt = _DT[x.dtype]
    ws_bytes = lib.dicp_normals_workspace_bytes(dt, N, m, k, c, 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    nrm = torch.empty((N, m, 3), dtype=x.dtype, device=x.device)
    walked = torch.zeros(N, dtype=torch.int64, device=x.device)
    _lib.check(lib.dicp_normals_forward(dt, _p(x), c, _p(rows), N, m, k, None, 0, _p(nrm), None, None, _p(ws), ws_bytes, _p(walked), _stream()),
               "dicp_normals_forward")
    return walked.sum().item() / (int(rows.sum()) if rows is not None else N * m)


def rows_scanned(x, k, rows=None):
    """mean rows fed to the list and boxes computed per query by one forward of the grid scan"""
    visited = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
    passes = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
    estimate_normals(x, k=k, rows=rows, method="grid", _visited=visited, _passes=passes)
    q = int(rows.sum()) if rows is not None else x.shape[0] * x.shape[1]
    return visited.sum().item() / q, passes.sum().item() / q


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


def measure(rec, pts, rows, ks, methods, reps):
    for k in ks:
        x = pts.clone().requires_grad_(True)
        g = torch.randn_like(pts[..., :3])

        def fb(method):
            x.grad = None
            (estimate_normals(x, k=k, rows=rows, method=method) * g).sum().backward()
        fwd = timed([lambda m=m: estimate_normals(pts, k=k, rows=rows, method=m) for m in methods], reps)
        fwdbwd = timed([lambda m=m: fb(m) for m in methods], reps)
        out = dict(rec, k=k)
        for m, f, fbm in zip(methods, fwd, fwdbwd):
            out["%s_fwd_ms" % m] = round(f, 3)
            out["%s_fwd_bwd_ms" % m] = round(fbm, 3)
        if "walk" in methods:
            out["rows_walked_per_query"] = round(rows_walked(pts, k, rows), 1)
        if "grid" in methods:
            v, p = rows_scanned(pts, k, rows)
            out["rows_visited_per_query"], out["boxes_per_query"] = round(v, 1), round(p, 2)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ks", default="8,16,32")
    ap.add_argument("--dtype", default="float32")
    ap.add_argument("--method", default="walk", help="walk, grid or walk,grid")
    ap.add_argument("--layouts", default="pairs,scene,wall")
    ap.add_argument("--downsampled", action="store_true", help="also voxel_downsample(--raw-points rows) -> estimate_normals(rows=), k = 16")
    ap.add_argument("--raw-points", type=int, default=131072)
    a = ap.parse_args()
    dtype = getattr(torch, a.dtype)
    methods = a.method.split(",")
    ks = [int(v) for v in a.ks.split(",")]
    gens = {"pairs": make_pairs, "scene": make_scene_pairs, "wall": make_wall_pairs}
    for name in [n for n in a.layouts.split(",") if n]:
        _, tgt = gens[name](a.clouds, 16, a.points, seed=1, dtype=dtype)
        pts = tgt[..., :3].contiguous().cuda()
        measure({"targets": name, "B": a.clouds, "m": a.points, "dtype": a.dtype}, pts, None, ks, methods, a.reps)
    if a.downsampled:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from voxel_bench import size_for
        from dicp_amd.voxel import voxel_downsample
        for name in ("scene", "pairs"):
            _, tgt = gens[name](a.clouds, 16, a.raw_points, seed=1, dtype=torch.float32)
            raw = tgt[..., :3].contiguous()
            cent, rows = voxel_downsample(raw.cuda(), size_for(raw[0].numpy()))
            measure({"targets": name + " downsampled", "B": a.clouds, "raw_m": a.raw_points, "M": cent.shape[1], "mean_rows": round(rows.float().mean().item(), 1),
                     "dtype": "float32"}, cent.detach(), rows, [16], methods, a.reps)


if __name__ == "__main__":
    main()
