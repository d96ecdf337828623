"""compute_fpfh at B = 256 x 16384 points, k in {8, 16, 32}, float32 and float64, on a uniform volume and on a planar scene: the two passes
on their own (dicp_fpfh_spfh, dicp_fpfh_combine), the whole compute_fpfh, the ball_query inside it -- and, in the same run on the same
clouds and the same idx, the torch composition a user would write without the operator: expanded gathers, atan2, scatter_add histograms,
chunked over the clouds to fit memory (float32 / float64 as the points; it is checked against the operator on the first chunk: the same
bins on all but the pairs that sit on a bin edge).  The radius is the one whose ball holds about k rows.  Every time is the median of --reps
calls after warm-up, each between two HIP events.  Beside them: the bytes each pass must move at least and their time at 8 TB/s, and the
double-precision instructions per pair of each kernel, counted in the disassembly (hipcc -S, device only).
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/fpfh_bench.py [--clouds 256] [--points 16384] [--reps 5]
-> profiles/r27_fpfh_bench.txt"""
import argparse
import json
import math
import os
import re
import statistics
import subprocess
import tempfile

import torch

from dicp_amd import _lib
from dicp_amd._ops import _DT, _p, _workspace
from dicp_amd.ball import ball_query
from dicp_amd.fpfh import compute_fpfh, fpfh_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    Nn = torch.randn((N, m, 3), generator=g, dtype=torch.float64)
    if layout == "planar":
        P[..., 2] = 0.02 * torch.sin(9.0 * P[..., 0]) * torch.cos(7.0 * P[..., 1])
        Nn = 0.3 * Nn + torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    Nn = Nn / Nn.norm(dim=-1, keepdim=True)
    return P.to(dtype).cuda(), Nn.to(dtype).cuda()


def radius_for(layout, m, k):
    """the radius whose ball holds about k of the m rows (unit cube / unit square)"""
    return (3.0 * k / (4.0 * math.pi * m)) ** (1.0 / 3.0) if layout == "uniform" else math.sqrt(k / (math.pi * m))


# ------------------------------------------------------------------ the torch composition
def torch_fpfh_chunk(P, Nn, idx, radius):
    """(C, m, 3), (C, m, 3), (C, m, k) -> (out (C, m, 33), cnt (C, m, 33)): the textbook formulas on expanded tensors"""
    C, m, k = idx.shape
    live = idx >= 0
    j = idx.clamp(min=0)
    b = torch.arange(C, device=P.device)[:, None, None]
    pj, nj = P[b, j], Nn[b, j]
    pi, ni = P[:, :, None, :], Nn[:, :, None, :].expand(-1, -1, k, -1)
    d = pj - pi
    r2 = (d * d).sum(-1)
    near = live & (j != torch.arange(m, device=P.device)[None, :, None]) & (r2 > 0) & (r2 <= radius * radius)
    r = r2.sqrt()
    a1, a2 = (ni * d).sum(-1) / r, (nj * d).sum(-1) / r
    swap = (a1.abs() < a2.abs())[..., None]
    n1, n2, d = torch.where(swap, nj, ni), torch.where(swap, ni, nj), torch.where(swap, -d, d)
    phi = torch.where(swap[..., 0], -a2, a1)
    v = torch.linalg.cross(d, n1)
    q = (v * v).sum(-1)
    v = v / q.sqrt()[..., None]
    w = torch.linalg.cross(n1, v)
    theta = torch.atan2((w * n2).sum(-1), (n1 * n2).sum(-1))
    alpha = (v * n2).sum(-1)
    pair = near & (q > 0)
    bt = (11.0 * (theta.nan_to_num(0.0) + math.pi) / (2.0 * math.pi)).floor().clamp(0, 10).long()
    ba = (11.0 * (alpha + 1.0) * 0.5).nan_to_num(0.0).floor().clamp(0, 10).long() + 11
    bp = (11.0 * (phi + 1.0) * 0.5).nan_to_num(0.0).floor().clamp(0, 10).long() + 22
    cnt = torch.zeros((C, m, 33), dtype=P.dtype, device=P.device)
    one = pair.to(P.dtype)
    for bins in (bt, ba, bp):
        cnt.scatter_add_(2, bins, one)
    c = pair.sum(-1, keepdim=True).to(P.dtype)
    s = torch.where(c > 0, 100.0 * cnt / c.clamp(min=1), torch.zeros_like(cnt))
    wj = torch.where(near, 1.0 / r2, torch.zeros_like(r2))
    acc = (wj[..., None] * s[b, j]).sum(2)
    S = acc.view(C, m, 3, 11).sum(-1, keepdim=True)
    out = torch.where(S != 0, 100.0 * acc.view(C, m, 3, 11) / S, torch.zeros_like(S)).reshape(C, m, 33) + s
    return out, cnt


def torch_fpfh(P, Nn, idx, radius, chunk):
    outs = [torch_fpfh_chunk(P[i:i + chunk], Nn[i:i + chunk], idx[i:i + chunk], radius)[0] for i in range(0, P.shape[0], chunk)]
    return torch.cat(outs)


# ------------------------------------------------------------------ the disassembly
def f64_counts():
    """double-precision vector instructions per kernel of csrc/fpfh.hip (static counts: pass 1 runs its body once per pair; pass 2's slot loop
    once per (row, slot)) -> {kernel: (all, v_rcp_f64)}; {} without hipcc"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        return {}
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "fpfh.s")
        subprocess.check_call([hipcc] + _lib.FLAGS + ["-I", os.path.join(ROOT, "include"), "--offload-device-only", "-S", "-o", asm,
                                                      os.path.join(ROOT, "dicp_amd", "csrc", "fpfh.hip")])
        text = open(asm).read()
    out = {}
    for name, body in re.findall(r"^(_Z\w*fpfh_\w+_kernel\w*):[^\n]*\n(.*?)s_endpgm", text, flags=re.S | re.M):
        short = ("spfh" if "spfh" in name else "combine") + (" float32" if "kernelIf" in name else " float64") + (" int64" if re.search(r"kernelI[fd]lE", name) else " int32")
        out[short] = (len(re.findall(r"^\s+v_\w+_f64", body, flags=re.M)), len(re.findall(r"^\s+v_rcp_f64", body, flags=re.M)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="8,16,32")
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_fpfh_bench.txt"))
    a = ap.parse_args()
    N, m = a.clouds, a.points
    lib = _lib.load()
    lines = []

    def emit(row):
        line = row if isinstance(row, str) else json.dumps(row)
        lines.append(line)
        print(line, flush=True)
    for layout in ("uniform", "planar"):
        for dtype in (torch.float32, torch.float64):
            P, Nn = clouds(layout, N, m, dtype)
            ts = 4 if dtype == torch.float32 else 8
            for k in [int(v) for v in a.ks.split(",")]:
                radius = radius_for(layout, m, k)
                idx = ball_query(P, P, radius, k=k)[1]
                ws_bytes = lib.dicp_fpfh_workspace_bytes(N, m)
                ws = _workspace(ws_bytes, P.device)
                out = torch.empty((N, m, 33), dtype=dtype, device=P.device)

                def pass1():
                    _lib.call("dicp_fpfh_spfh", P.device, _DT[dtype], _p(P), 3, _p(Nn), _p(idx), 1, None, N, m, k, radius, _p(ws), ws_bytes, None)

                def pass2():
                    _lib.call("dicp_fpfh_combine", P.device, _DT[dtype], _p(P), 3, _p(idx), 1, None, N, m, k, radius, _p(ws), ws_bytes, _p(out))
                t1, t2 = timed(pass1, a.reps), timed(pass2, a.reps)
                t_ball = timed(lambda: ball_query(P, P, radius, k=k), a.reps)
                t_all = timed(lambda: compute_fpfh(P, Nn, radius, k=k), a.reps)
                t_torch = timed(lambda: torch_fpfh(P, Nn, idx, radius, a.chunk), a.reps)
                # the check of the composition: the same counts except on bin edges
                got, spfh = fpfh_features(P[:a.chunk], Nn[:a.chunk], idx[:a.chunk], radius=radius, return_spfh=True)
                want, cnt = torch_fpfh_chunk(P[:a.chunk], Nn[:a.chunk], idx[:a.chunk], radius)
                rows_same = (spfh.to(cnt.dtype) == cnt).all(-1).float().mean().item()
                pairs = int((idx >= 0).sum().item())
                b1 = N * m * k * 8 + N * m * 6 * ts + N * m * 48
                b2 = N * m * k * 8 + N * m * 3 * ts + N * m * 48 + N * m * 33 * ts
                emit({"layout": layout, "dtype": str(dtype).replace("torch.", ""), "B": N, "m": m, "k": k, "radius": round(radius, 5),
                      "slots_filled": round(pairs / (N * m * k), 3), "spfh_ms": round(t1, 3), "combine_ms": round(t2, 3),
                      "ball_query_ms": round(t_ball, 3), "compute_fpfh_ms": round(t_all, 3), "ball_share": round(t_ball / t_all, 3),
                      "torch_composition_ms": round(t_torch, 3), "torch_over_passes": round(t_torch / (t1 + t2), 2),
                      "spfh_floor_ms_at_8TBs": round(b1 / 8e12 * 1e3, 3), "combine_floor_ms_at_8TBs": round(b2 / 8e12 * 1e3, 3),
                      "torch_rows_with_the_same_counts": round(rows_same, 4),
                      "torch_max_abs_diff_on_those_rows": round(float((got - want).abs()[(spfh.to(cnt.dtype) == cnt).all(-1)].max().item()), 6)})
                del idx, ws, out
            del P, Nn
            torch.cuda.empty_cache()
    counts = f64_counts()
    for name, (n, div) in sorted(counts.items()):
        emit("# kernel %s: %d v_*_f64 instructions, %d of them v_rcp_f64, one per division (static counts.  spfh: its body runs once per pair; "
             "combine: half in the slot loop, once per (row, slot), half in the epilogue, once per row)" % (name, n, div))
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
