"""select_rows against the torch composition a user writes without it, and the two outlier filters end to end: median of --reps calls after
2 warm-ups, HIP events, profiler off, at 256 clouds x 16384 and 256 x 131072 points, float32 and float64.
  select lines   c in {3, 6}, keep ratios 0.5 / 0.95 / 1.0 (a random mask per cloud).  In the same run, one after the other:
    sel_fwd_ms / sel_fb_ms       select_rows forward, and forward + backward (torch.autograd.grad of a random cotangent)
    torch_fwd_ms / torch_fb_ms   the composition: a stable argsort of ~mask, gather with the expanded index, zeroing the tail
    floor_ms                     the bytes a compaction must move -- the points and the mask read once, the output written once -- at 8 TB/s
  filter lines   c = 3, the unit cube with 1 % of the rows moved far out:
    ms / search_ms / search_share   the filter end to end, its search alone (ball_query with counts / knn_points with k + 1 slots), the share
No ratio is fixed in advance: every line is printed, the slower ones included.
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/filter_bench.py | tee profiles/r22_filter_bench.txt"""
import argparse
import json
import os
import statistics
import sys

import torch

from dicp_amd.ball import ball_query
from dicp_amd.filter import radius_outlier_removal, select_rows, statistical_outlier_removal
from dicp_amd.knn import knn_points

PEAK_BYTES_PER_MS = 8e12 / 1e3


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


def torch_select(x, mask):
    """what a user writes today: (out (N,m,c) zero past the kept rows, rows_out (N))"""
    N, m, c = x.shape
    order = torch.argsort(~mask, dim=1, stable=True)
    out = torch.gather(x, 1, order.unsqueeze(-1).expand(-1, -1, c))
    n = mask.sum(1)
    tail = torch.arange(m, device=x.device).unsqueeze(0) >= n.unsqueeze(1)
    return out.masked_fill(tail.unsqueeze(-1), 0), n.to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--rows", nargs="+", type=int, default=[16384, 131072])
    ap.add_argument("--dtypes", nargs="+", default=["float32", "float64"])
    ap.add_argument("--cols", nargs="+", type=int, default=[3, 6])
    ap.add_argument("--keep", nargs="+", type=float, default=[0.5, 0.95, 1.0])
    ap.add_argument("--skip-filters", action="store_true")
    a = ap.parse_args()
    N, dev = a.clouds, "cuda"
    print("# " + " ".join(sys.argv), flush=True)
    import dicp_amd
    print("# %s, torch %s, package %s" % (torch.cuda.get_device_name(0), torch.__version__, os.path.relpath(os.path.dirname(dicp_amd.__file__))), flush=True)
    gen = torch.Generator(device=dev).manual_seed(1)
    for m in a.rows:
        for dname in a.dtypes:
            dtype = getattr(torch, dname)
            ts = torch.empty((), dtype=dtype).element_size()
            for c in a.cols:
                pts = torch.rand((N, m, c), generator=gen, device=dev, dtype=dtype)
                g = torch.randn((N, m, c), generator=gen, device=dev, dtype=dtype)
                for keep in a.keep:
                    mask = torch.rand((N, m), generator=gen, device=dev) < keep
                    line = {"op": "select_rows", "dtype": dname, "clouds": N, "rows": m, "c": c, "keep": keep}

                    def fb(f):
                        x = pts.detach().requires_grad_(True)
                        return torch.autograd.grad(f(x, mask)[0], [x], [g])[0]
                    ref, got = torch_select(pts, mask), select_rows(pts, mask)
                    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])
                    assert torch.equal(fb(torch_select), fb(select_rows))
                    del ref, got
                    line["sel_fwd_ms"] = round(timed(lambda: select_rows(pts, mask), a.reps), 3)
                    line["sel_fb_ms"] = round(timed(lambda: fb(select_rows), a.reps), 3)
                    line["torch_fwd_ms"] = round(timed(lambda: torch_select(pts, mask), a.reps), 3)
                    line["torch_fb_ms"] = round(timed(lambda: fb(torch_select), a.reps), 3)
                    line["floor_ms"] = round((2 * N * m * c * ts + N * m) / PEAK_BYTES_PER_MS, 3)
                    line["torch_over_sel_fwd"] = round(line["torch_fwd_ms"] / line["sel_fwd_ms"], 2)
                    line["torch_over_sel_fb"] = round(line["torch_fb_ms"] / line["sel_fb_ms"], 2)
                    print(json.dumps(line), flush=True)
                del pts, g
                torch.cuda.empty_cache()
            if a.skip_filters:
                continue
            pts = torch.rand((N, m, 3), generator=gen, device=dev, dtype=dtype)
            pts[:, ::100] += 2.0 + torch.rand((N, pts[:, ::100].shape[1], 3), generator=gen, device=dev, dtype=dtype)
            radius = 2.0 * (1.0 / m) ** (1.0 / 3.0)                 # about 33 rows of the cube in a ball
            for name, run, search in (
                    ("radius_outlier_removal", lambda: radius_outlier_removal(pts, radius, 8), lambda: ball_query(pts, pts, radius, k=1, return_counts=True)),
                    ("statistical_outlier_removal", lambda: statistical_outlier_removal(pts, k=16, std_ratio=2.0), lambda: knn_points(pts, pts, 17, method="grid"))):
                line = {"op": name, "dtype": dname, "clouds": N, "rows": m, "c": 3}
                line["kept"] = round(float(run()[1].sum()) / (N * m), 4)
                line["ms"] = round(timed(run, a.reps), 3)
                line["search_ms"] = round(timed(search, a.reps), 3)
                line["search_share"] = round(line["search_ms"] / line["ms"], 3)
                print(json.dumps(line), flush=True)
            del pts
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
