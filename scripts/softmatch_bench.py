"""soft_match_features (dicp_amd/match.py) against what a user writes without it, on one MI355X: medians of --reps calls after a warm-up,
HIP events, profiler off, at --clouds x --rows x --rows (32 x 16384 x 16384), C = 3, every sample printed.
  forward                 D in {32, 64, 128}, float32 in both forms (_form="mfma" / "valu"); one float64 line at D = 32
  forward + backward      out.sum().backward() into fx, fy and values (default form)
Beside each line, in the same run:
  knn_ms                  knn_features(k=1) on the same tables: the same matrix-core work without the softmax
  torch_ms                the per-cloud loop  torch.softmax(-torch.cdist(x, y) ** 2 / tau, -1) @ values  -- it forms the (n, m) matrix, 1 GB per
                          cloud in float32, and keeps it for the backward; one cloud at a time so that it fits
  tflops, pct_peak        2 N n m D / time of the forward, and its share of the float32 matrix / vector peak (157.3 TF: both are
                          64 FLOP / clk / SIMD); for float64 the share of the float64 vector peak (78.6 TF, the public datasheet figure)
No time is fixed in advance.
Run from the repo root: PYTHONPATH=. python scripts/softmatch_bench.py [--reps 5] | tee profiles/r28_softmatch_bench.txt"""
import argparse
import json
import statistics

import torch

from dicp_amd.match import knn_features, soft_match_features

PEAK_TF = {torch.float32: 157.3, torch.float64: 78.6}


def timed(fn, reps, warmup=1):
    """(median, samples) of reps calls (ms), each between two HIP events"""
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
        ts.append(round(a.elapsed_time(b), 3))
    return statistics.median(ts), ts


def torch_soft(x, y, v, tau):
    """what a user writes today, cloud by cloud -> out (N, n, C)"""
    return torch.stack([torch.softmax(-torch.cdist(x[b], y[b]) ** 2 / tau, -1) @ v[b] for b in range(x.shape[0])])


def torch_soft_backward(x, y, v, tau):
    """forward + backward of the same, cloud by cloud (one cloud's matrix alive at a time)"""
    for b in range(x.shape[0]):
        (torch.softmax(-torch.cdist(x[b], y[b]) ** 2 / tau, -1) @ v[b]).sum().backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--tau", type=float, default=0.5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    N, n, C, tau = a.clouds, a.rows, 3, a.tau
    print(json.dumps({"device": torch.cuda.get_device_name(0), "clouds": N, "rows": n, "C": C, "tau": tau, "reps": a.reps}))
    g = torch.Generator(device=dev).manual_seed(0)
    for dtype, Ds in ((torch.float32, (32, 64, 128)), (torch.float64, (32,))):
        for D in Ds:
            y = torch.randn(N, n, D, device=dev, dtype=dtype, generator=g) / D ** 0.5
            x = y[:, torch.randperm(n, device=dev)] + 0.2 * torch.randn(N, n, D, device=dev, dtype=dtype, generator=g) / D ** 0.5
            v = torch.rand(N, n, C, device=dev, dtype=dtype, generator=g)
            flop = 2.0 * N * n * n * D
            knn_ms, knn_s = timed(lambda: knn_features(x, y, k=1), a.reps)
            t_ms, t_s = timed(lambda: torch_soft(x, y, v, tau), a.reps)
            for form in (("mfma", "valu") if dtype == torch.float32 else (None,)):
                ms, s = timed(lambda: soft_match_features(x, y, v, tau, _form=form), a.reps)
                print(json.dumps({"what": "forward", "dtype": str(dtype)[6:], "D": D, "form": form or "valu", "ms": round(ms, 3), "samples": s,
                                  "knn_ms": round(knn_ms, 3), "knn_samples": knn_s, "torch_ms": round(t_ms, 3), "torch_samples": t_s,
                                  "vs_knn": round(ms / knn_ms, 2), "vs_torch": round(ms / t_ms, 3),
                                  "tflops": round(flop / ms * 1e-9, 3), "pct_peak": round(100 * flop / ms * 1e-9 / PEAK_TF[dtype], 3)}), flush=True)
            xg, yg, vg = (t.clone().requires_grad_(True) for t in (x, y, v))

            def both():
                xg.grad = yg.grad = vg.grad = None
                soft_match_features(xg, yg, vg, tau).sum().backward()

            def torch_both():
                xg.grad = yg.grad = vg.grad = None
                torch_soft_backward(xg, yg, vg, tau)
            ms, s = timed(both, a.reps)
            tb_ms, tb_s = timed(torch_both, a.reps)
            print(json.dumps({"what": "forward+backward", "dtype": str(dtype)[6:], "D": D, "ms": round(ms, 3), "samples": s, "torch_ms": round(tb_ms, 3),
                              "torch_samples": tb_s, "vs_torch": round(ms / tb_ms, 3)}), flush=True)
            del x, y, v, xg, yg, vg


if __name__ == "__main__":
    main()
