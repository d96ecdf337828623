"""pool_neighbors against the two compositions a user can write without it: forward and forward + backward (median of --reps calls after 2
warm-ups, HIP events, profiler off) at 256 clouds in float32 with C = 1, 3, 64 and every reduce:
  centres              1024 centres x k = 16 out of 16384 rows;
  every point          16384 queries x k = 16 out of 16384 rows.
Indices are uniformly random rows (no locality: the pessimistic case for the gathers), one slot in eight empty (-1).  Three paths in the same
run, one after the other per line:
  pool      pool_neighbors(f, idx, reduce)
  group     group_points(f, idx) -> masked reduce over the k slots
  torch     clamp -> expanded gather -> mask -> reduce: no operator of this package
bwd_ms is the DIFFERENCE of the two medians (the backward is not timed on its own).  Beside each line: fwd_floor_ms, the bytes the forward
has to move (every gathered row once, the indices, out, argmax for the maximum, counts) over 8 TB/s, and fwd_of_floor = floor / measured;
atomic_floor_ms, the bytes the backward adds (n C elements for the maximum, the live slots' rows otherwise) over 1.3 TB/s.
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/pool_bench.py [--reps 5] | tee profiles/r17_pool_bench.txt"""
import argparse
import json
import statistics
import sys

import torch

from dicp_amd.group import group_points, pool_neighbors

HBM, ATOMIC = 8e12, 1.3e12           # bytes / s
WAVE = 64


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


def reduce_slots(x, live, reduce):
    """(N, n, k, C) with its mask (N, n, k) -> (N, n, C); queries without a live slot give 0"""
    m = live[..., None]
    if reduce == "max":
        return torch.where(live.any(2)[..., None], x.masked_fill(~m, float("-inf")).amax(2), torch.zeros((), dtype=x.dtype, device=x.device))
    s = (x * m).sum(2)
    return s if reduce == "sum" else s / live.sum(2, keepdim=True).clamp(min=1)


def via_group(f, idx, reduce):
    return reduce_slots(group_points(f, idx), idx >= 0, reduce)


def via_torch(f, idx, reduce):
    N, n, k = idx.shape
    C = f.shape[2]
    x = torch.gather(f, 1, idx.clamp(min=0).reshape(N, n * k, 1).expand(-1, -1, C)).reshape(N, n, k, C)
    return reduce_slots(x, idx >= 0, reduce)


def lane_occupancy(C, ts=4):
    """lanes with work / 64 of the wide forward (None: the narrow form): G lanes per query hold C * ts / 16 packs"""
    if C * ts < 128:
        return None
    packs = C * ts // 16 if (C * ts) % 16 == 0 else C
    g = 8
    while g < min(packs, WAVE):
        g *= 2
    return round((packs / g) if packs <= WAVE else packs / (g * -(-packs // g)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--centres", type=int, default=1024)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 3, 64])
    a = ap.parse_args()
    N, dev, ts, k, m = a.clouds, "cuda", 4, a.k, a.rows
    print("# " + " ".join(sys.argv), flush=True)
    print("# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__), flush=True)
    gen = torch.Generator(device=dev).manual_seed(1)
    slower = []
    for n in (a.centres, a.rows):
        for C in a.channels:
            f = torch.randn((N, m, C), generator=gen, device=dev).requires_grad_(True)
            idx = torch.randint(0, m, (N, n, k), generator=gen, device=dev)
            idx = torch.where(torch.randint(0, 8, (N, n, k), generator=gen, device=dev) == 0, torch.full_like(idx, -1), idx)
            g = torch.randn((N, n, C), generator=gen, device=dev)
            Q, live = N * n, int((idx >= 0).sum())
            for reduce in ("max", "mean", "sum"):
                def fb(fn):
                    def run():
                        f.grad = None
                        fn(f, idx, reduce).backward(g)
                    return run
                rec = {"n": n, "m": m, "k": k, "C": C, "N": N, "reduce": reduce, "form": "wide" if C * ts >= 128 else "narrow"}
                for name, fn in (("pool", pool_neighbors), ("group", via_group), ("torch", via_torch)):
                    with torch.no_grad():
                        fwd = timed(lambda: fn(f, idx, reduce), a.reps)
                    both = timed(fb(fn), a.reps)
                    rec.update({name + "_fwd_ms": round(fwd, 3), name + "_fwd_bwd_ms": round(both, 3), name + "_bwd_ms": round(both - fwd, 3)})
                    f.grad = None
                    torch.cuda.empty_cache()
                fwd_bytes = live * C * ts + Q * k * 8 + Q * C * ts + (Q * C * 4 if reduce == "max" else 0) + Q * 4
                added = (Q * C if reduce == "max" else live * C) * ts
                rec.update({"fwd_speedup_vs_group": round(rec["group_fwd_ms"] / rec["pool_fwd_ms"], 2), "fwd_speedup_vs_torch": round(rec["torch_fwd_ms"] / rec["pool_fwd_ms"], 2),
                            "fwd_bwd_speedup_vs_group": round(rec["group_fwd_bwd_ms"] / rec["pool_fwd_bwd_ms"], 2),
                            "fwd_bwd_speedup_vs_torch": round(rec["torch_fwd_bwd_ms"] / rec["pool_fwd_bwd_ms"], 2),
                            "fwd_MB": round(fwd_bytes / 1e6, 1), "fwd_floor_ms": round(fwd_bytes / HBM * 1e3, 4), "fwd_of_floor": round(fwd_bytes / HBM / (rec["pool_fwd_ms"] * 1e-3), 3),
                            "atomic_MB": round(added / 1e6, 1), "atomic_floor_ms": round(added / ATOMIC * 1e3, 4), "wide_lane_occupancy": lane_occupancy(C, ts)})
                for other in ("group", "torch"):
                    for what in ("fwd_ms", "fwd_bwd_ms"):
                        if rec["pool_" + what] >= rec[other + "_" + what]:
                            slower.append("n=%d C=%d %s %s: pool %.3f >= %s %.3f" % (n, C, reduce, what, rec["pool_" + what], other, rec[other + "_" + what]))
                print(json.dumps(rec), flush=True)
            del f, idx, g
            torch.cuda.empty_cache()
    print("# lines where pool_neighbors was not faster: %s" % (slower if slower else "none"), flush=True)


if __name__ == "__main__":
    main()
