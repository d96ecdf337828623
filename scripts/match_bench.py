"""knn_features / match_features (dicp_amd/match.py) against what a user writes without them, on one MI355X: medians of --reps calls
after a warm-up, HIP events, profiler off, at --clouds x --rows x --rows (32 x 16384 x 16384), every line printed.
  forward                 D in {32, 64, 128} x k in {1, 2, 8}, float32 in both forms (_form="mfma" / "valu"); float64 at D = 32
  forward + backward      d2.sum().backward() into fx and fy, the default (float atomics) and deterministic=True, default form
  match_features          mutual=True, ratio=0.8 as a whole (a k = 2 search, the reverse k = 1 search, the rules)
Beside each line, in the same run:
  torch_ms                the per-cloud loop  torch.cdist(x, y).pow(2).topk(k, largest=False)  -- it forms the (n, m) matrix, 1 GB per cloud
                          in float32 (for match_features: that loop with k = 2, the reverse loop with k = 1 and the same rules)
  tflops, pct_peak        2 N n m D / time of the search, and its share of the float32 matrix / vector peak (157.3 TF: both are
                          64 FLOP / clk / SIMD); for float64 the share of the float64 vector peak (78.6 TF, the public datasheet figure)
No time is fixed in advance; the lines on which the library call is not the faster one are listed again at the end.
Run from the repo root: PYTHONPATH=. python scripts/match_bench.py [--reps 5] | tee profiles/r25_match_bench.txt"""
import argparse
import json
import statistics

import torch

from dicp_amd.match import knn_features, match_features

PEAK_TF = {torch.float32: 157.3, torch.float64: 78.6}


def timed(fn, reps, warmup=1):
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


def torch_knn(x, y, k):
    """what a user writes today, cloud by cloud -> d2 (N, n, k), idx (N, n, k)"""
    out = [torch.cdist(x[b], y[b]).pow(2).topk(k, largest=False) for b in range(x.shape[0])]
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


def torch_match(x, y, ratio):
    d2, idx = torch_knn(x, y, 2)
    _, back = torch_knn(y, x, 1)
    keep = (d2[..., 0] <= ratio * ratio * d2[..., 1]) & (torch.gather(back[..., 0], 1, idx[..., 0]) == torch.arange(x.shape[1], device=x.device)[None])
    return torch.where(keep, idx[..., 0], torch.full_like(idx[..., 0], -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--rows", type=int, default=16384)
    a = ap.parse_args()
    dev = torch.device("cuda")
    N, n = a.clouds, a.rows
    gen = torch.Generator(device=dev).manual_seed(0)
    print("# %s, %d clouds x %d x %d rows, median of %d" % (torch.cuda.get_device_name(0), N, n, n, a.reps))
    slower = []

    def line(**kw):
        if "ms" in kw and "torch_ms" in kw and not kw["ms"] < kw["torch_ms"]:
            slower.append(kw)
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in kw.items()}), flush=True)

    for dtype, dims in ((torch.float32, (32, 64, 128)), (torch.float64, (32,))):
        for D in dims:
            y = torch.randn((N, n, D), generator=gen, device=dev, dtype=dtype)
            x = y[:, torch.randperm(n, generator=gen, device=dev)] + 0.1 * torch.randn((N, n, D), generator=gen, device=dev, dtype=dtype)
            flop = 2.0 * N * n * n * D
            name = str(dtype).replace("torch.", "")
            for k in (1, 2, 8):
                t_torch = timed(lambda: torch_knn(x, y, k), a.reps)
                for form in (("mfma", "valu") if dtype == torch.float32 else ("valu",)):
                    ms = timed(lambda: knn_features(x, y, k, _form=form), a.reps)
                    line(what="forward", dtype=name, D=D, k=k, form=form, ms=ms, torch_ms=t_torch, tflops=flop / ms * 1e-9, pct_peak=100 * flop / ms * 1e-9 / PEAK_TF[dtype])
                if dtype == torch.float32:
                    fx, fy = x.clone().requires_grad_(True), y.clone().requires_grad_(True)

                    def both(det):
                        fx.grad = fy.grad = None
                        knn_features(fx, fy, k, deterministic=det)[0].sum().backward()
                    for det in (False, True):
                        line(what="forward+backward", dtype=name, D=D, k=k, deterministic=det, ms=timed(lambda: both(det), a.reps))
            if dtype == torch.float32:
                line(what="match_features mutual ratio=0.8", dtype=name, D=D, ms=timed(lambda: match_features(x, y, mutual=True, ratio=0.8), a.reps),
                     torch_ms=timed(lambda: torch_match(x, y, 0.8), a.reps))
            del x, y
    print("# lines on which the library call is not faster than the torch loop: %d" % len(slower))
    for kw in slower:
        print("#   " + json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in kw.items()}))


if __name__ == "__main__":
    main()
