"""The deterministic backward of estimate_normals (deterministic=True) against the atomic one, and its parts: median of --reps calls after
2 warm-ups, HIP events, profiler off, at 256 clouds x 16384 points, float32 and float64, k in {8, 16, 32}, method "walk" and "grid".
Layouts, every cloud its own sample: uniform (the unit cube), planar (z within 1e-3), wall (x within 1e-3), and dup -- the unit cube
with 1 % of the rows exact copies of one row per cloud (164 copies: lists of up to 164 k entries at those rows, whose own queries have
a zero covariance and so carry no term).  Per line, in the same run, one after the other:
  fwd_ms                        the forward (the same kernels and bytes with and without the keyword)
  atomic_bwd_ms / det_bwd_ms    the backward alone (torch.autograd.grad on a kept graph): the default, and deterministic=True -- the
                                records pass, the index build, the gather
  atomic_fb_ms / det_fb_ms      forward + backward
  records_ms / build_ms / gather_ms   the three parts of the deterministic backward alone (dicp_normals_backward_records,
                                dicp_invert_neighbors, dicp_normals_gather_det)
No ratio is fixed in advance: every line is printed, the slower ones included.
  --default-only   the forward and forward + backward of the default call alone, without the keyword: also runs on the commit before
                   the feature (PYTHONPATH), to show that the default path did not move
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/normals_det_bench.py [--reps 5] | tee profiles/r21_normals_det_bench.txt"""
import argparse
import json
import os
import statistics
import sys

import torch

from dicp_amd.normals import estimate_normals

LAYOUTS = ("uniform", "planar", "wall", "dup")


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


def cloud(layout, N, n, dtype, gen, dev):
    x = torch.rand((N, n, 3), generator=gen, device=dev, dtype=torch.float64)
    if layout == "planar":
        x[..., 2] *= 1e-3
    elif layout == "wall":
        x[..., 0] *= 1e-3
    elif layout == "dup":
        x[:, ::100] = x[:, :1]
    return x.to(dtype).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--layouts", nargs="+", default=list(LAYOUTS))
    ap.add_argument("--ks", nargs="+", type=int, default=[8, 16, 32])
    ap.add_argument("--dtypes", nargs="+", default=["float32", "float64"])
    ap.add_argument("--methods", nargs="+", default=["walk", "grid"])
    ap.add_argument("--default-only", action="store_true")
    a = ap.parse_args()
    N, n, dev = a.clouds, a.rows, "cuda"
    print("# " + " ".join(sys.argv), flush=True)
    import dicp_amd
    print("# %s, torch %s, package %s" % (torch.cuda.get_device_name(0), torch.__version__, os.path.relpath(os.path.dirname(dicp_amd.__file__))), flush=True)
    gen = torch.Generator(device=dev).manual_seed(1)
    for dname in a.dtypes:
        dtype = getattr(torch, dname)
        for layout in a.layouts:
            pts = cloud(layout, N, n, dtype, gen, dev)
            gn = torch.randn((N, n, 3), generator=gen, device=dev, dtype=dtype)
            gc = torch.randn((N, n), generator=gen, device=dev, dtype=dtype)
            for k in a.ks:
                for method in a.methods:
                    line = {"dtype": dname, "layout": layout, "k": k, "method": method, "clouds": N, "rows": n}

                    def fwd(x, **kw):
                        return estimate_normals(x, k=k, return_curvature=True, method=method, **kw)

                    def fb(**kw):
                        x = pts.detach().requires_grad_(True)
                        return torch.autograd.grad(fwd(x, **kw), [x], [gn, gc])[0]
                    line["fwd_ms"] = round(timed(lambda: fwd(pts), a.reps), 3)
                    line["atomic_fb_ms"] = round(timed(fb, a.reps), 3)
                    if not a.default_only:
                        from dicp_amd import _lib
                        from dicp_amd._ops import _DT, _p
                        from dicp_amd.group import _invert
                        for key, kw in (("atomic", {}), ("det", {"deterministic": True})):
                            x = pts.detach().requires_grad_(True)
                            outs = fwd(x, **kw)
                            line[key + "_bwd_ms"] = round(timed(lambda: torch.autograd.grad(outs, [x], [gn, gc], retain_graph=True), a.reps), 3)
                            del outs, x
                        line["det_fb_ms"] = round(timed(lambda: fb(deterministic=True), a.reps), 3)
                        recs = []
                        x = pts.detach().requires_grad_(True)
                        outs = estimate_normals(x, k=k, return_curvature=True, method=method, deterministic=True, _records=recs)
                        node = outs[0].grad_fn
                        torch.autograd.grad(outs, [x], [gn, gc], retain_graph=True)
                        rec, nbr_o = recs[0]
                        ws = node.ws
                        line["records_ms"] = round(timed(lambda: _lib.call("dicp_normals_backward_records", pts.device, _DT[dtype], int(method == "grid"), _p(gn), _p(gc), None, 0, None,
                                                                           N, n, k, 3, _p(ws), ws.numel(), _p(rec), _p(nbr_o)), a.reps), 3)
                        line["build_ms"] = round(timed(lambda: _invert(nbr_o, None, n), a.reps), 3)
                        off, slots = _invert(nbr_o, None, n)
                        grad = torch.empty((N, n, 3), dtype=dtype, device=dev)
                        line["gather_ms"] = round(timed(lambda: _lib.call("dicp_normals_gather_det", pts.device, _DT[dtype], _p(rec), _p(nbr_o), 0, None, N, n, k, 3, _p(off), _p(slots),
                                                                          _p(grad)), a.reps), 3)
                        line["max_list"] = int((off[:, 1:] - off[:, :-1]).max())
                        line["det_over_atomic_bwd"] = round(line["det_bwd_ms"] / line["atomic_bwd_ms"], 2)
                        line["det_over_atomic_fb"] = round(line["det_fb_ms"] / line["atomic_fb_ms"], 3)
                        del outs, x, node, rec, nbr_o, ws, off, slots, grad, recs
                    print(json.dumps(line), flush=True)
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
