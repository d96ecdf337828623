"""The deterministic backward of group_points / pool_neighbors / interpolate_features against the atomic one, and invert_neighbors on its
own: the BACKWARD alone (torch.autograd.grad on a kept graph; median of --reps calls after 2 warm-ups, HIP events, profiler off) at 256
clouds in float32 with C = 1, 3, 64:
  group_points          1024 centres x k = 16 out of 16384 rows;
  pool_neighbors        1024 and 16384 queries x k = 16 out of 16384 rows, every reduce;
  interpolate_features  16384 rows x k = 3 out of 1024 centres.
Indices are uniformly random rows, one slot in eight empty (-1), as scripts/group_bench.py and scripts/pool_bench.py.  Per line, in the
same run, one after the other:
  atomic_ms        the backward into the features with float atomics (the default)
  det_ms           deterministic=True: the index build inside the backward, then the gather over the lists
  det_prebuilt_ms  inverse=: the gather alone
  build_ms         invert_neighbors alone (it does not depend on C or on the operator: timed per line all the same)
and beside them atomic_floor_ms, the bytes the atomic backward adds over 1.3 TB/s, and store_floor_ms, the table's bytes -- what the
deterministic form stores -- over 5.85 TB/s (4.5 x the atomic rate: DESIGN.md section 8, item 10(a)).
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/group_det_bench.py [--reps 5] | tee profiles/r19_group_det_bench.txt"""
import argparse
import json
import statistics
import sys

import torch

from dicp_amd.group import group_points, interpolate_features, invert_neighbors, pool_neighbors

ATOMIC, STORE = 1.3e12, 5.85e12      # bytes / s


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--centres", type=int, default=1024)
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 3, 64])
    a = ap.parse_args()
    N, dev, ts = a.clouds, "cuda", 4
    print("# " + " ".join(sys.argv), flush=True)
    print("# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__), flush=True)
    gen = torch.Generator(device=dev).manual_seed(1)
    slower = []

    def indices(n, k, m):
        idx = torch.randint(0, m, (N, n, k), generator=gen, device=dev)
        return torch.where(torch.randint(0, 8, (N, n, k), generator=gen, device=dev) == 0, torch.full_like(idx, -1), idx)

    def line(op, reduce, C, n, m, k, idx, forward, g, added):
        """forward(f, **kw) -> the operator's output on a fresh leaf f"""
        f = torch.randn((N, m, C), generator=gen, device=dev).requires_grad_(True)
        inv = invert_neighbors(idx, m)
        rec = {"op": op, "reduce": reduce, "N": N, "n": n, "m": m, "k": k, "C": C, "form": "wide" if C * ts >= 128 else "narrow"}
        for name, kw in (("atomic_ms", {}), ("det_ms", {"deterministic": True}), ("det_prebuilt_ms", {"inverse": inv})):
            out = forward(f, **kw)
            rec[name] = round(timed(lambda: torch.autograd.grad(out, [f], g, retain_graph=True), a.reps), 3)
            del out
        rec["build_ms"] = round(timed(lambda: invert_neighbors(idx, m), a.reps), 3)
        deg = (inv[0][:, 1:] - inv[0][:, :-1])
        rec.update({"det_over_atomic": round(rec["det_ms"] / rec["atomic_ms"], 2), "det_prebuilt_over_atomic": round(rec["det_prebuilt_ms"] / rec["atomic_ms"], 2),
                    "atomic_MB": round(added / 1e6, 1), "atomic_floor_ms": round(added / ATOMIC * 1e3, 4),
                    "store_MB": round(N * m * C * ts / 1e6, 1), "store_floor_ms": round(N * m * C * ts / STORE * 1e3, 4),
                    "in_degree_mean": round(float(deg.float().mean()), 2), "in_degree_max": int(deg.max())})
        for name in ("det_ms", "det_prebuilt_ms"):
            if rec[name] >= rec["atomic_ms"]:
                slower.append("%s %s n=%d C=%d: %s %.3f >= atomic %.3f" % (op, reduce or "", n, C, name, rec[name], rec["atomic_ms"]))
        print(json.dumps(rec), flush=True)
        del f, inv
        torch.cuda.empty_cache()

    for C in a.channels:
        n, m, k = a.centres, a.rows, 16
        idx = indices(n, k, m)
        live = int((idx >= 0).sum())
        g4 = torch.randn((N, n, k, C), generator=gen, device=dev)
        line("group_points", None, C, n, m, k, idx, lambda f, **kw: group_points(f, idx, **kw), g4, live * C * ts)
        del g4
        for n in (a.centres, a.rows):
            if n != a.centres:
                idx = indices(n, k, m)
                live = int((idx >= 0).sum())
            g = torch.randn((N, n, C), generator=gen, device=dev)
            for reduce in ("max", "mean", "sum"):
                line("pool_neighbors", reduce, C, n, m, k, idx, lambda f, **kw: pool_neighbors(f, idx, reduce, **kw), g, (N * n * C if reduce == "max" else live * C) * ts)
            del g
        n, m, k = a.rows, a.centres, 3
        idx = indices(n, k, m)
        live = int((idx >= 0).sum())
        d2 = torch.rand((N, n, k), generator=gen, device=dev) + 0.01
        g = torch.randn((N, n, C), generator=gen, device=dev)
        line("interpolate_features", None, C, n, m, k, idx, lambda f, **kw: interpolate_features(f, idx, d2, eps=1e-8, **kw), g, live * C * ts)
        del idx, d2, g
        torch.cuda.empty_cache()
    print("# lines where the deterministic backward was not faster than the atomic one: %s" % (slower if slower else "none"), flush=True)


if __name__ == "__main__":
    main()
