"""compute_iss_keypoints at B = 256 x 16384 points, k in {8, 16, 32}, float32 and float64, on a uniform volume and on a planar scene: the two
passes on their own (dicp_iss_saliency, dicp_iss_maxima), the whole compute_iss_keypoints, the ball_query inside it -- and, in the same
run on the same clouds and the same idx, the torch composition a user would write without the operator: clamp, expanded gather, batched
covariance, torch.linalg.eigvalsh, gathered saliency compare, chunked over the clouds to fit memory and timed on --torch-clouds of the
clouds (its time for all B is that times B / --torch-clouds; it is checked against the operator on the first chunk).  The radius is the
one whose ball holds about k rows.  Every time is the median of --reps calls after warm-up, each between two HIP events.  Beside them:
the bytes each pass must move at least -- idx once, k gathered rows, the outputs -- and their time at 8 TB/s.
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/iss_bench.py [--clouds 256] [--points 16384] [--reps 5]
-> profiles/r31_iss_bench.txt"""
import argparse
import json
import math
import os
import statistics

import torch

from dicp_amd import _lib
from dicp_amd._ops import _DT, _p, _workspace
from dicp_amd.ball import ball_query
from dicp_amd.iss import compute_iss_keypoints, iss_keypoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G21 = G32 = 0.975
MIN_NB = 5


def timed(fn, reps, warmup=1):
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


def clouds(layout, N, m, dtype, seed=1):
    g = torch.Generator().manual_seed(seed)
    P = torch.rand((N, m, 3), generator=g, dtype=torch.float64)
    if layout == "planar":
        P[..., 2] = 0.02 * torch.sin(9.0 * P[..., 0]) * torch.cos(7.0 * P[..., 1])
    return P.to(dtype).cuda()


def radius_for(layout, m, k):
    """the radius whose ball holds about k of the m rows (unit cube / unit square)"""
    return (3.0 * k / (4.0 * math.pi * m)) ** (1.0 / 3.0) if layout == "uniform" else math.sqrt(k / (math.pi * m))


# ------------------------------------------------------------------ the torch composition
def torch_iss_chunk(P, idx, radius):
    """(C, m, 3), (C, m, k) -> (saliency (C, m), mask (C, m)): the textbook formulas on expanded tensors, both passes under ONE radius.
    With one radius and one idx the member count of the suppression is the count of the saliency pass, which the saliency rule has
    already held to MIN_NB, so the mask needs no count test of its own; with two radii or an nms_idx it would."""
    C, m, k = idx.shape
    ar = torch.arange(m, device=P.device)[None, :, None]
    b = torch.arange(C, device=P.device)[:, None, None]
    live = (idx >= 0) & (idx != ar)
    j = idx.clamp(min=0)
    q = P[b, j] - P[:, :, None, :]
    mem = live & ((q * q).sum(-1) <= radius * radius)
    w = mem.to(P.dtype)[..., None]
    cnt = 1 + mem.sum(-1)
    n = cnt.to(P.dtype)[..., None]
    mu = (q * w).sum(2) / n
    d = (q - mu[:, :, None, :]) * w
    cov = (torch.einsum("cmki,cmkj->cmij", d, d) + mu[..., :, None] * mu[..., None, :]) / n[..., None]
    lam = torch.linalg.eigvalsh(cov)
    good = (cnt >= MIN_NB) & (lam[..., 1] < G21 * lam[..., 2]) & (lam[..., 0] > 0) & (lam[..., 0] < G32 * lam[..., 1])
    sal = torch.where(good, lam[..., 0], torch.zeros_like(lam[..., 0]))
    si, sj = sal[..., None], sal[b, j]
    beats = mem & ((sj > si) | ((sj == si) & (j < ar)))
    return sal, (sal > 0) & ~beats.any(-1)


def torch_iss(P, idx, radius, chunk):
    return [torch_iss_chunk(P[i:i + chunk], idx[i:i + chunk], radius) for i in range(0, P.shape[0], chunk)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="8,16,32")
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--torch-clouds", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_iss_bench.txt"))
    a = ap.parse_args()
    N, m = a.clouds, a.points
    tc = min(a.torch_clouds, N)
    lib = _lib.load()
    lines = []

    def emit(row):
        line = row if isinstance(row, str) else json.dumps(row)
        lines.append(line)
        print(line, flush=True)
        with open(a.out, "w") as fh:                        # (every line as soon as it is measured)
            fh.write("\n".join(lines) + "\n")
    for layout in ("uniform", "planar"):
        for dtype in (torch.float32, torch.float64):
            P = clouds(layout, N, m, dtype)
            ts = 4 if dtype == torch.float32 else 8
            for k in [int(v) for v in a.ks.split(",")]:
                radius = radius_for(layout, m, k)
                idx = ball_query(P, P, radius, k=k)[1]
                ws_bytes = lib.dicp_iss_workspace_bytes(N, m)
                ws = _workspace(ws_bytes, P.device)
                sal = torch.empty((N, m), dtype=dtype, device=P.device)
                mask = torch.empty((N, m), dtype=torch.bool, device=P.device)

                def pass1():
                    _lib.call("dicp_iss_saliency", P.device, _DT[dtype], _p(P), 3, _p(idx), 1, None, N, m, k, radius, G21, G32, MIN_NB, _p(ws), ws_bytes,
                              _p(sal), None, None)

                def pass2():
                    _lib.call("dicp_iss_maxima", P.device, _DT[dtype], _p(P), 3, _p(idx), 1, None, N, m, k, radius, MIN_NB, _p(ws), ws_bytes, _p(mask))
                t1, t2 = timed(pass1, a.reps), timed(pass2, a.reps)
                t_ball = timed(lambda: ball_query(P, P, radius, k=k), a.reps)
                t_all = timed(lambda: compute_iss_keypoints(P, radius, k=k), a.reps)
                t_torch = timed(lambda: torch_iss(P[:tc], idx[:tc], radius, a.chunk), a.reps)
                # the check of the composition on the first chunk: the same decisions except at rounding distance of a threshold
                got_mask, got_sal = iss_keypoints(P[:a.chunk], idx[:a.chunk], salient_radius=radius, non_max_radius=radius, return_saliency=True)
                want_sal, want_mask = torch_iss_chunk(P[:a.chunk], idx[:a.chunk], radius)
                both = (got_sal > 0) & (want_sal > 0)
                rel = ((got_sal - want_sal).abs() / want_sal.abs().clamp(min=1e-300))[both]
                slots = int((idx >= 0).sum().item())
                b1 = N * m * k * 8 + N * m * k * 3 * ts + N * m * (8 + ts)
                b2 = N * m * k * 8 + N * m * k * (3 * ts + 8) + N * m
                emit({"layout": layout, "dtype": str(dtype).replace("torch.", ""), "B": N, "m": m, "k": k, "radius": round(radius, 5),
                      "slots_filled": round(slots / (N * m * k), 3), "salient_share": round(float((sal > 0).float().mean().item()), 4),
                      "keypoints_per_cloud": round(float(mask.sum().item()) / N, 1),
                      "saliency_ms": round(t1, 3), "maxima_ms": round(t2, 3), "ball_query_ms": round(t_ball, 3),
                      "compute_iss_keypoints_ms": round(t_all, 3), "ball_share": round(t_ball / t_all, 3),
                      "torch_composition_ms_for_%d_clouds" % tc: round(t_torch, 3), "torch_composition_ms_scaled_to_B": round(t_torch * N / tc, 1),
                      "torch_over_passes": round(t_torch * N / tc / (t1 + t2), 1),
                      "saliency_floor_ms_at_8TBs": round(b1 / 8e12 * 1e3, 3), "maxima_floor_ms_at_8TBs": round(b2 / 8e12 * 1e3, 3),
                      "torch_rows_with_the_same_mask": round(float((got_mask == want_mask).float().mean().item()), 5),
                      "torch_rows_with_the_same_salient_decision": round(float(((got_sal > 0) == (want_sal > 0)).float().mean().item()), 5),
                      "torch_max_rel_diff_of_saliency": float("%.3g" % (rel.max().item() if rel.numel() else 0.0))})
                del idx, ws, sal, mask
            del P
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
