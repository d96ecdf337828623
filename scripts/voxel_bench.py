"""voxel_downsample: forward and forward + backward (median of --reps calls after warm-up, HIP events, profiler off) at 256 x 131072 float32 on
make_scene_pairs and make_pairs targets, with voxel sizes chosen for about 8x fewer points, and at 1 x 4194304 (a single map); then
estimate_normals(k=16) on the raw and on the downsampled clouds (the neighbour walk's cost against local density).  HBM bytes per kernel
family are computed from the shapes (model_bytes).
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/voxel_bench.py [--reps 10] [--normals-reps 2] [--skip-normals]
-> profiles/r08_voxel_bench.txt"""
import argparse
import json
import statistics

import numpy as np
import torch

from dicp_amd.normals import estimate_normals
from dicp_amd.synthetic import make_pairs, make_scene_pairs
from dicp_amd.voxel import voxel_downsample


def timed(fn, reps, warmup=2):
    """median of reps calls (ms), each between two HIP events"""
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


def size_for(P, ratio=8.0):
    """a voxel size that gives about `ratio` points per voxel on the (m, 3) numpy cloud P (bisection on the log of the size)"""
    lo, hi = 1e-3, 10.0
    for _ in range(30):
        s = (lo * hi) ** 0.5
        n = np.unique(np.floor(P / np.float32(s)).astype(np.int64), axis=0).shape[0]
        if P.shape[0] / n < ratio:
            lo = s
        else:
            hi = s
    return float(np.float32((lo * hi) ** 0.5))


def model_bytes(N, m, V, c, ts, passes):
    """HBM bytes per kernel family from shapes (the radix passes move key + row index in and out; reads of the rows by index are
    counted once per row)"""
    rows = N * m
    return {"bounds": rows * 3 * ts, "keys": rows * 3 * ts + rows * 12, "sort": passes * rows * (12 + 12 + 8),
            "segments": rows * 8 * 2 + V * 4 * 2, "reduce": rows * (4 + c * ts + 8) + V * (c * ts + 4 + 12) + rows * 8,
            "backward": rows * (8 + c * ts) + rows * c * ts + V * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--normals-reps", type=int, default=2)
    ap.add_argument("--skip-normals", action="store_true")
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--map-points", type=int, default=4194304)
    a = ap.parse_args()
    cases = []
    for name, gen in (("scene", make_scene_pairs), ("pairs", make_pairs)):
        _, tgt = gen(a.clouds, 16, a.points, seed=1, dtype=torch.float32)
        pts = tgt[..., :3].contiguous()
        cases.append((name, pts, size_for(pts[0].numpy())))
    g = torch.Generator().manual_seed(21)
    m = a.map_points
    xy = (torch.rand((m, 2), generator=g, dtype=torch.float64) - 0.5) * 200.0
    z = 0.5 * torch.sin(0.1 * xy[:, :1]) + 0.05 * torch.randn((m, 1), generator=g, dtype=torch.float64)
    mp = torch.cat((xy, z), 1).to(torch.float32).unsqueeze(0)
    cases.append(("map", mp, 0.3))                         # (a 200 m x 200 m surface: about 8 points per 0.3 m voxel)
    for name, pts, size in cases:
        x = pts.cuda()
        N, m, c = x.shape
        cent, rows = voxel_downsample(x, size)
        V = int(rows.sum())
        fwd = timed(lambda: voxel_downsample(x, size), a.reps)
        xg = x.clone().requires_grad_(True)
        gc = torch.randn_like(cent)

        def fb():
            xg.grad = None
            c_, _ = voxel_downsample(xg, size)
            (c_ * gc).sum().backward()
        fwdbwd = timed(fb, a.reps)
        rec = {"targets": name, "N": N, "m": m, "voxel": size, "voxels": V, "points_per_voxel": round(N * m / V, 2), "fwd_ms": round(fwd, 3),
               "fwd_bwd_ms": round(fwdbwd, 3), "bwd_ms": round(fwdbwd - fwd, 3)}
        ext = [float(v) for v in (x.amax((0, 1)) - x.amin((0, 1))).cpu()]
        bits = sum(int(np.ceil(e / size)).bit_length() for e in ext)
        mb = model_bytes(N, m, V, c, 4, (bits + 7) // 8)
        rec["model_fwd_GB"] = round(sum(v for k, v in mb.items() if k != "backward") / 1e9, 3)
        rec["model_bytes"] = mb
        if not a.skip_normals and name != "map":
            raw = timed(lambda: estimate_normals(x, k=16), a.normals_reps, warmup=1)
            down = timed(lambda: estimate_normals(cent, k=16, rows=rows), a.reps)
            rec.update({"normals_raw_ms": round(raw, 3), "normals_down_ms": round(down, 3), "down_M": cent.shape[1]})
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
