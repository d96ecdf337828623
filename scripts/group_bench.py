"""group_points and interpolate_features: forward and forward + backward (median of --reps calls after 2 warm-ups, HIP events,
profiler off) at 256 clouds in float32 with C = 1, 3, 64:
  grouping             1024 centres x k = 16 out of 16384 rows;
  interpolation        16384 rows x k = 3 out of 1024 centres.
Indices are uniformly random rows (no locality: the pessimistic case for the gathers), one slot in eight empty (-1).  Beside each number, in
the same run, the same result from torch ops -- clamp, expanded gather, mask, weighted sum: the composition a user writes today, not a tuned
baseline.  bwd_ms is the DIFFERENCE of the two medians (the backward is not timed on its own).  bytes: what the algorithm has to move (the
index, every gathered row once, the output; for a backward the cotangent, the zero fill and the added bytes), as a fraction of 8 TB/s over the
measured time; atomic_floor_ms: the added bytes over the 1.3 TB/s the chip adds at, whatever the schedule.
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/group_bench.py [--reps 5]
-> profiles/r15_group_bench.txt"""
import argparse
import json
import statistics

import torch

from dicp_amd.group import group_points, interpolate_features

HBM, ATOMIC = 8e12, 1.3e12           # bytes / s


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


def torch_gather(f, idx):
    """(N, m, C), (N, n, k) -> the masked (N, n, k, C) and the mask"""
    N, n, k = idx.shape
    C = f.shape[2]
    live = idx >= 0
    out = torch.gather(f, 1, idx.clamp(min=0).reshape(N, n * k, 1).expand(-1, -1, C)).reshape(N, n, k, C)
    return out, live


def torch_group(f, idx):
    out, live = torch_gather(f, idx)
    return out * live[..., None]


def torch_interp(f, idx, d2, eps):
    out, live = torch_gather(f, idx)
    r = torch.where(live, 1.0 / (d2 + eps), torch.zeros_like(d2))
    w = r / r.sum(2, keepdim=True).clamp(min=1e-30)
    return (out * w[..., None]).sum(2)


def both(ours, theirs, leaves, g, reps):
    """fwd and fwd + bwd medians of the operator and of the torch composition; leaves: the tensors whose gradients are wanted"""
    def fb(fn):
        def run():
            for t in leaves:
                t.grad = None
            fn().backward(g)
        return run
    with torch.no_grad():
        f1, f2 = timed(ours, reps), timed(theirs, reps)
    return f1, timed(fb(ours), reps), f2, timed(fb(theirs), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--centres", type=int, default=1024)
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 3, 64])
    a = ap.parse_args()
    N, dev, ts = a.clouds, "cuda", 4
    gen = torch.Generator(device=dev).manual_seed(1)

    def indices(n, k, m):
        idx = torch.randint(0, m, (N, n, k), generator=gen, device=dev)
        return torch.where(torch.randint(0, 8, (N, n, k), generator=gen, device=dev) == 0, torch.full_like(idx, -1), idx)

    def line(op, C, n, m, k, times, fwd_bytes, bwd_bytes, added):
        f1, fb1, f2, fb2 = times
        b1, b2 = fb1 - f1, fb2 - f2
        rec = {"op": op, "N": N, "n": n, "m": m, "k": k, "C": C, "form": "wide" if C * ts >= 128 else "narrow",
               "fwd_ms": round(f1, 3), "fwd_bwd_ms": round(fb1, 3), "bwd_ms": round(b1, 3),
               "torch_fwd_ms": round(f2, 3), "torch_fwd_bwd_ms": round(fb2, 3), "torch_bwd_ms": round(b2, 3),
               "fwd_speedup": round(f2 / f1, 2), "fwd_bwd_speedup": round(fb2 / fb1, 2),
               "fwd_MB": round(fwd_bytes / 1e6, 1), "fwd_of_8TBs": round(fwd_bytes / HBM / (f1 * 1e-3), 3),
               "bwd_MB": round(bwd_bytes / 1e6, 1), "bwd_of_8TBs": round(bwd_bytes / HBM / (max(b1, 1e-6) * 1e-3), 3),
               "atomic_MB": round(added / 1e6, 1), "atomic_floor_ms": round(added / ATOMIC * 1e3, 3)}
        print(json.dumps(rec), flush=True)

    for C in a.channels:
        # grouping: n centres x 16 slots out of `rows` rows
        n, m, k = a.centres, a.rows, 16
        f = torch.randn((N, m, C), generator=gen, device=dev).requires_grad_(True)
        idx = indices(n, k, m)
        Q, live = N * n, int((idx >= 0).sum())
        g = torch.randn((N, n, k, C), generator=gen, device=dev)
        t = both(lambda: group_points(f, idx), lambda: torch_group(f, idx), [f], g, a.reps)
        line("group_points", C, n, m, k, t, Q * k * 8 + live * C * ts + Q * k * C * ts, Q * k * C * ts + Q * k * 8 + N * m * C * ts + live * C * ts, live * C * ts)
        del f, idx, g
        # interpolation: `rows` rows x 3 slots out of n centres
        n, m, k = a.rows, a.centres, 3
        f = torch.randn((N, m, C), generator=gen, device=dev).requires_grad_(True)
        idx = indices(n, k, m)
        d2 = (torch.rand((N, n, k), generator=gen, device=dev) + 0.01).requires_grad_(True)
        Q, live = N * n, int((idx >= 0).sum())
        g = torch.randn((N, n, C), generator=gen, device=dev)
        t = both(lambda: interpolate_features(f, idx, d2, eps=1e-8), lambda: torch_interp(f, idx, d2, 1e-8), [f, d2], g, a.reps)
        line("interpolate_features", C, n, m, k, t, Q * k * (8 + ts) + live * C * ts + Q * C * ts,
             2 * Q * C * ts + Q * k * (8 + 2 * ts) + live * C * ts + N * m * C * ts + live * C * ts, live * C * ts)
        del f, idx, d2, g


if __name__ == "__main__":
    main()
