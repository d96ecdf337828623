"""knn_points and chamfer_distance, method="walk" against method="grid", at B = 256 x 16384 queries against 16384 rows, k = 1, 8 and 32:
the whole call forward and forward + backward, the grid build on its own, the mean rows visited and passes made per query by the grid
search (and the rows walked by the walk), in the same process on the same clouds, the two methods taking turns call by call.  On
make_pairs (uniform volume) and make_scene_pairs (planar) clouds and on a wall perpendicular to x, the slow case of the x-sorted walk;
float32, and float64 at --points64 rows.  Every time is the median of --reps calls after warm-up, each between two HIP events, profiler
off.  The clouds, the warm-up and the timing are scripts/ball_query_bench.py's.
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/grid_knn_bench.py [--clouds 256] [--points 16384] [--reps 5]
-> profiles/r13_grid_knn_bench.txt"""
import argparse
import json

import torch

from ball_query_bench import make_wall_pairs, rows_walked, timed
from dicp_amd.ball import CellGrid
from dicp_amd.knn import chamfer_distance, knn_points
from dicp_amd.synthetic import make_pairs, make_scene_pairs


def grid_counters(x, y, k):
    """mean rows visited and passes made per query by one grid search (the library's diagnostic counters)"""
    visited = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
    passes = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
    knn_points(x, y, k=k, method="grid", _visited=visited, _passes=passes)
    q = x.shape[0] * x.shape[1]
    return visited.sum().item() / q, passes.sum().item() / q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--points64", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="1,8,32")
    a = ap.parse_args()
    gens = {"pairs": make_pairs, "scene": make_scene_pairs, "wall": make_wall_pairs}
    for dtype, points, names in ((torch.float32, a.points, tuple(gens)), (torch.float64, a.points64, ("pairs",))):
        for name in names:
            src, tgt = gens[name](a.clouds, points, points, seed=1)
            x = src[..., :3].contiguous().to(dtype).cuda()
            y = tgt[..., :3].contiguous().to(dtype).cuda()
            xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
            for k in [int(v) for v in a.ks.split(",")]:
                g = torch.randn((a.clouds, points, k), device=x.device, dtype=dtype)

                def fb(method):
                    def run():
                        xg.grad = yg.grad = None
                        (knn_points(xg, yg, k=k, method=method)[0] * g).sum().backward()
                    return run
                wf, gf, wfb, gfb, build = timed([lambda: knn_points(x, y, k=k), lambda: knn_points(x, y, k=k, method="grid"), fb("walk"), fb("grid"),
                                                 lambda: CellGrid.by_density(y, None)], a.reps)
                rows, passes = grid_counters(x, y, k)
                row = {"clouds": name, "dtype": str(dtype).split(".")[1], "B": a.clouds, "n": points, "m": points, "k": k,
                       "walk_fwd_ms": round(wf, 3), "grid_fwd_ms": round(gf, 3), "walk_fwd_bwd_ms": round(wfb, 3), "grid_fwd_bwd_ms": round(gfb, 3),
                       "grid_build_ms": round(build, 3), "grid_rows_visited_per_query": round(rows, 1), "grid_passes_per_query": round(passes, 2),
                       "walk_rows_walked_per_query": round(rows_walked(x, y, k), 1)}
                print(json.dumps(row), flush=True)

            def cfb(method):
                def run():
                    xg.grad = yg.grad = None
                    chamfer_distance(xg, yg, method=method).backward()
                return run
            wf, gf, wfb, gfb = timed([lambda: chamfer_distance(x, y), lambda: chamfer_distance(x, y, method="grid"), cfb("walk"), cfb("grid")], a.reps)
            print(json.dumps({"clouds": name, "dtype": str(dtype).split(".")[1], "B": a.clouds, "n": points, "m": points, "chamfer_walk_fwd_ms": round(wf, 3),
                              "chamfer_grid_fwd_ms": round(gf, 3), "chamfer_walk_fwd_bwd_ms": round(wfb, 3), "chamfer_grid_fwd_bwd_ms": round(gfb, 3)}), flush=True)


if __name__ == "__main__":
    main()
