"""The deterministic y-gradient of knn_points / ball_query / chamfer_distance (deterministic=True) against the atomic one: the BACKWARD
alone (torch.autograd.grad on a kept graph) and forward + backward, median of --reps calls after 2 warm-ups, HIP events, profiler off,
at 256 clouds x 16384 points each side in float32:
  chamfer_distance      method="walk" and "grid" (two k = 1 searches);
  knn_points            k = 8, method="grid";
  ball_query            k = 8, a radius that holds about eight rows.
Layouts, every cloud its own sample: uniform (the unit cube), planar (z within 1e-3), wall (x within 1e-3), and hub -- the queries in
the unit cube, 16 of the targets (rows 7, 1031, 2055, ...: spread over the cloud) on a lattice inside it and all the others a cube's
width away, so that every query's nearest targets are among those 16 rows (in-degree about 1024 k: lists of 16 k chunks; in Chamfer's
other direction the far targets share the queries next to them).  Per line, in the same run, one after the other:
  atomic_ms / det_ms           the default, and deterministic=True: the index build inside the backward, then the gather
  *_bwd_ms / *_fwd_bwd_ms      the backward alone / forward + backward
and, per layout, build_ms: dicp_invert_neighbors alone on the k = 1 and the k = 8 index tensor.  No ratio is fixed in advance: every
line is printed, the slower ones listed again at the end.
  --default-only   the default (atomic) lines of chamfer_distance and ball_query alone, without the keyword: also runs on the commit
                   before the feature (PYTHONPATH), to show that the default path did not move
  --sweep TAG      the KNN_DET_HUB sweep: the deterministic backward of chamfer_distance (walk) on uniform and hub, tagged TAG; run
                   once per build of the library (DICP_HIP_LIB), KNN_DET_HUB = 2, 4, 8, 16
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/knn_det_bench.py [--reps 5] | tee profiles/r20_knn_det_bench.txt"""
import argparse
import json
import statistics
import sys

import torch

from dicp_amd.ball import ball_query
from dicp_amd.knn import chamfer_distance, knn_points

LAYOUTS = ("uniform", "planar", "wall", "hub")
RADIUS = {"uniform": 0.049, "planar": 0.0125, "wall": 0.0125, "hub": 0.6}      # about eight rows in the ball (hub: the 16 lattice rows' spacing)


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


def clouds(layout, N, n, gen, dev):
    """-> x, y (N, n, 3) float32"""
    x, y = torch.rand((N, n, 3), generator=gen, device=dev), torch.rand((N, n, 3), generator=gen, device=dev)
    if layout == "planar":
        x[..., 2] *= 1e-3
        y[..., 2] *= 1e-3
    elif layout == "wall":
        x[..., 0] *= 1e-3
        y[..., 0] *= 1e-3
    elif layout == "hub":
        y += 2.0
        t = torch.arange(16, device=dev)
        y[:, 7::n // 16][:, :16] = torch.stack([(t % 4).float() / 4 + 0.125, ((t // 4) % 2).float() / 2 + 0.25, (t // 8).float() / 2 + 0.25], 1)[None] + 0.01 * torch.rand((N, 16, 3), generator=gen, device=dev)
    return x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--layouts", nargs="+", default=list(LAYOUTS))
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--sweep", default=None)
    a = ap.parse_args()
    N, n, dev = a.clouds, a.rows, "cuda"
    print("# " + " ".join(sys.argv), flush=True)
    print("# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__), flush=True)
    gen = torch.Generator(device=dev).manual_seed(1)
    slower = []

    def line(op, layout, forward, modes, x0, y0, g, extra=None):
        """forward(x, y, **kw) -> the tensor to differentiate"""
        rec = dict({"op": op, "layout": layout, "N": N, "n": n}, **(extra or {}))
        for name, kw in modes:
            x, y = x0.clone().requires_grad_(True), y0.clone().requires_grad_(True)
            out = forward(x, y, **kw)
            rec[name + "_bwd_ms"] = round(timed(lambda: torch.autograd.grad(out, [x, y], g, retain_graph=True), a.reps), 3)
            del out

            def both():
                o = forward(x, y, **kw)
                torch.autograd.grad(o, [x, y], g)
            rec[name + "_fwd_bwd_ms"] = round(timed(both, a.reps), 3)
        if len(modes) == 2:
            for part in ("bwd", "fwd_bwd"):
                rec["det_over_atomic_" + part] = round(rec["det_%s_ms" % part] / rec["atomic_%s_ms" % part], 2)
                if rec["det_%s_ms" % part] >= rec["atomic_%s_ms" % part]:
                    slower.append("%s %s %s: det %.3f >= atomic %.3f" % (op, layout, part, rec["det_%s_ms" % part], rec["atomic_%s_ms" % part]))
        print(json.dumps(rec), flush=True)

    both_modes = (("atomic", {}), ("det", {"deterministic": True}))
    for layout in a.layouts:
        x0, y0 = clouds(layout, N, n, gen, dev)
        g8 = torch.randn((N, n, 8), generator=gen, device=dev)
        if a.sweep is not None:
            if layout in ("uniform", "hub"):
                line("chamfer_distance walk", layout, lambda x, y, **kw: chamfer_distance(x, y, method="walk", **kw), (("det", {"deterministic": True}),), x0, y0, None, {"KNN_DET_HUB": a.sweep})
            continue
        modes = (("atomic", {}),) if a.default_only else both_modes
        for meth in ("walk", "grid"):
            line("chamfer_distance " + meth, layout, lambda x, y, **kw: chamfer_distance(x, y, method=meth, **kw), modes, x0, y0, None)
        if not a.default_only:
            line("knn_points k=8 grid", layout, lambda x, y, **kw: knn_points(x, y, k=8, method="grid", **kw)[0], modes, x0, y0, g8)
        line("ball_query k=8", layout, lambda x, y, **kw: ball_query(x, y, RADIUS[layout], k=8, **kw)[0], modes, x0, y0, g8, {"radius": RADIUS[layout]})
        if not a.default_only:
            from dicp_amd.group import _invert
            rec = {"op": "invert_neighbors", "layout": layout, "N": N, "n": n}
            for k in (1, 8):
                idx = knn_points(x0, y0, k=k, method="grid")[1].contiguous()
                rec["build_k%d_ms" % k] = round(timed(lambda: _invert(idx, None, n), a.reps), 3)
                off = _invert(idx, None, n)[0]
                rec["in_degree_max_k%d" % k] = int((off[:, 1:] - off[:, :-1]).max())
                del idx, off
            print(json.dumps(rec), flush=True)
        del x0, y0, g8
        torch.cuda.empty_cache()
    if a.sweep is None and not a.default_only:
        print("# lines where deterministic=True was not faster than the default: %s" % (slower if slower else "none"), flush=True)


if __name__ == "__main__":
    main()
