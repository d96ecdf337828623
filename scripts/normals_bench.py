"""estimate_normals at B = 256 x 16384: forward and forward + backward per k, on make_pairs targets (uniform volume) and on make_scene_pairs
targets (planar; two walls perpendicular to x, the sorted walk's slow case), with the mean number of rows the walk visits per query.
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/normals_bench.py [--clouds 256] [--points 16384] [--reps 10]
-> profiles/r07_normals_bench.txt"""
import argparse
import ctypes
import json

import torch

from dicp_amd import _lib
from dicp_amd._ops import _DT, _p, _stream
from dicp_amd.normals import estimate_normals
from dicp_amd.synthetic import make_pairs, make_scene_pairs


def rows_walked(x, k):
    """mean rows visited per query by one forward (the library's diagnostic counters)"""
    N, m, c = x.shape
    lib = _lib.load()
    dt = _DT[x.dtype]
    ws_bytes = lib.dicp_normals_workspace_bytes(dt, N, m, k, c, 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    nrm = torch.empty((N, m, 3), dtype=x.dtype, device=x.device)
    walked = torch.zeros(N, dtype=torch.int64, device=x.device)
    _lib.check(lib.dicp_normals_forward(dt, _p(x), c, None, N, m, k, None, 0, _p(nrm), None, None, _p(ws), ws_bytes, _p(walked), _stream()),
               "dicp_normals_forward")
    return walked.sum().item() / (N * m)


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
    ap.add_argument("--ks", default="8,16,32")
    ap.add_argument("--dtype", default="float32")
    a = ap.parse_args()
    dtype = getattr(torch, a.dtype)
    gens = {"pairs": make_pairs, "scene": make_scene_pairs}
    for name, gen in gens.items():
        _, tgt = gen(a.clouds, 16, a.points, seed=1, dtype=dtype)
        pts = tgt[..., :3].contiguous().cuda()
        for k in [int(v) for v in a.ks.split(",")]:
            fwd = timed(lambda: estimate_normals(pts, k=k), a.reps)
            x = pts.clone().requires_grad_(True)
            g = torch.randn_like(pts)

            def fb():
                x.grad = None
                (estimate_normals(x, k=k) * g).sum().backward()
            fwdbwd = timed(fb, a.reps)
            print(json.dumps({"targets": name, "B": a.clouds, "m": a.points, "k": k, "dtype": a.dtype, "fwd_ms": round(fwd, 3),
                              "fwd_bwd_ms": round(fwdbwd, 3), "rows_walked_per_query": round(rows_walked(pts, k), 1)}), flush=True)


if __name__ == "__main__":
    main()
