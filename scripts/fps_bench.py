"""sample_farthest_points: forward and forward + backward (median of --reps calls after warm-up, HIP events, profiler off) at 256 x 16384 in
float32 (the resident form) and float64 (beyond float64's resident limit: the streamed form) with k = 1024 and k = 4096, at 256 x 8192 float64
(resident), and at 256 x 131072 float32 with k = 1024 (streamed).  Beside
each number, the same sampling written as a loop of torch ops on the same device (torch_fps below: per step one gather of the pick, one
(N, n) distance pass, a minimum, an argmax) -- the comparison a user has today, not a tuned baseline.  bwd_ms is the DIFFERENCE of the two
medians fwd_bwd_ms - fwd_ms (the backward is not timed on its own): within the run-to-run spread of the forward it can come out negative.
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/fps_bench.py [--reps 5]
-> profiles/r11_fps_bench.txt"""
import argparse
import json
import statistics

import torch

from dicp_amd import fps
from dicp_amd.fps import sample_farthest_points
from dicp_amd.synthetic import make_pairs


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


def torch_fps(x, k):
    """the k-step loop in torch ops: (N, n, c) -> (picked rows (N, k, c), idx (N, k)); start row 0, ties to the lowest index"""
    N, n, c = x.shape
    ar = torch.arange(N, device=x.device)
    D = torch.full((N, n), float("inf"), dtype=x.dtype, device=x.device)
    pick = torch.zeros(N, dtype=torch.int64, device=x.device)
    idx = torch.empty((N, k), dtype=torch.int64, device=x.device)
    xyz = x[..., :3]
    for t in range(k):
        idx[:, t] = pick
        d = ((xyz - xyz[ar, pick][:, None]) ** 2).sum(-1)
        D = torch.minimum(D, d)
        D[ar, pick] = -1
        pick = D.argmax(1)
    return torch.gather(x, 1, idx[..., None].expand(-1, -1, c)), idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--big-points", type=int, default=131072)
    ap.add_argument("--skip-torch", action="store_true")
    a = ap.parse_args()
    cases = [(a.points, torch.float32, 1024), (a.points, torch.float32, 4096), (a.points, torch.float64, 1024), (a.points, torch.float64, 4096), (a.points // 2, torch.float64, 1024),
             (a.big_points, torch.float32, 1024)]
    clouds = {}
    for n, dtype, k in cases:
        if n not in clouds:
            clouds[n] = make_pairs(a.clouds, 16, n, seed=1, dtype=torch.float32)[1][..., :3].contiguous()
        x = clouds[n].to(dtype).cuda()
        N = x.shape[0]
        fwd = timed(lambda: sample_farthest_points(x, k), a.reps)
        xg = x.clone().requires_grad_(True)
        g = torch.randn((N, k, 3), dtype=dtype, device=x.device)

        def fb():
            xg.grad = None
            p, _ = sample_farthest_points(xg, k)
            p.backward(g)
        fwdbwd = timed(fb, a.reps)
        rec = {"N": N, "n": n, "dtype": str(dtype).replace("torch.", ""), "k": k, "form": "resident" if n <= fps.NR[dtype] else "streamed",
               "fwd_ms": round(fwd, 3), "fwd_bwd_ms": round(fwdbwd, 3), "bwd_ms": round(fwdbwd - fwd, 3), "us_per_step": round(1e3 * fwd / k, 3)}
        if not a.skip_torch:
            tl = timed(lambda: torch_fps(x, k), a.reps, warmup=1)
            same = bool(torch.equal(torch_fps(x, k)[1], sample_farthest_points(x, k)[1]))
            rec.update({"torch_loop_ms": round(tl, 3), "torch_loop_us_per_step": round(1e3 * tl / k, 3), "speedup": round(tl / fwd, 2),
                        "torch_loop_same_picks": same})
        print(json.dumps(rec), flush=True)
        del x, xg, g


if __name__ == "__main__":
    main()
