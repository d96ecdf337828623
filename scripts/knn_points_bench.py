"""knn_points / chamfer_distance at B = 256 x 16384 queries against 16384 targets (float32): knn_points forward and forward + backward at
k = 1, 8, 16, chamfer_distance forward + backward, and -- in the same process, on the same clouds -- nn.nn_index in both directions as the
baseline; with the mean number of rows the walk visits per query, on make_pairs (uniform volume), make_scene_pairs (planar) and
make_independent_pairs clouds.
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/knn_points_bench.py [--clouds 256] [--points 16384] [--reps 10]
-> profiles/r09_knn_points_bench.txt"""
import argparse
import json

import torch

from dicp_amd import _lib
from dicp_amd._ops import _DT, _p, _stream
from dicp_amd.knn import _Prepared, chamfer_distance, knn_points
from dicp_amd.nn import nn
from dicp_amd.synthetic import make_independent_pairs, make_pairs, make_scene_pairs


def rows_walked(x, y, k):
    """mean rows visited per query by one search (the library's diagnostic counters)"""
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


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ks", default="1,8,16")
    a = ap.parse_args()
    gens = {"pairs": make_pairs, "scene": make_scene_pairs, "independent": lambda *a, **kw: make_independent_pairs(*a, ragged=False, **kw)}
    for name, gen in gens.items():
        src, tgt = gen(a.clouds, a.points, a.points, seed=1)
        x = src[..., :3].contiguous().cuda()
        y = tgt[..., :3].contiguous().cuda()
        finder = nn(differentiable=False)
        base_xy = timed(lambda: finder.nn_index(x, y), a.reps)
        base_yx = timed(lambda: finder.nn_index(y, x), a.reps)
        for k in [int(v) for v in a.ks.split(",")]:
            fwd = timed(lambda: knn_points(x, y, k=k), a.reps)
            xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
            g = torch.randn((a.clouds, a.points, k), device=x.device)

            def fb():
                xg.grad = yg.grad = None
                (knn_points(xg, yg, k=k)[0] * g).sum().backward()
            fwdbwd = timed(fb, a.reps)
            print(json.dumps({"clouds": name, "B": a.clouds, "n": a.points, "m": a.points, "k": k, "op": "knn_points", "fwd_ms": round(fwd, 3),
                              "fwd_bwd_ms": round(fwdbwd, 3), "rows_walked_per_query": round(rows_walked(x, y, k), 1),
                              "nn_index_x_to_y_ms": round(base_xy, 3), "nn_index_y_to_x_ms": round(base_yx, 3)}), flush=True)
        xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        cf = timed(lambda: chamfer_distance(x, y), a.reps)

        def cfb():
            xg.grad = yg.grad = None
            chamfer_distance(xg, yg).backward()
        cfwdbwd = timed(cfb, a.reps)
        print(json.dumps({"clouds": name, "B": a.clouds, "n": a.points, "m": a.points, "op": "chamfer_distance", "fwd_ms": round(cf, 3),
                          "fwd_bwd_ms": round(cfwdbwd, 3), "rows_walked_per_query_y_to_x": round(rows_walked(y, x, 1), 1),
                          "nn_index_both_directions_ms": round(base_xy + base_yx, 3)}), flush=True)


if __name__ == "__main__":
    main()
