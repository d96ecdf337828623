"""Whole-ball normals (estimate_normals_ball: dicp_normals_ball_forward / _records / _gather on the cloud's cell grid), pass by pass, beside
the two yardsticks measured in the same run on the same clouds: B = 256 x 16384 points, a uniform volume and a planar scene, float32 and
float64 (the set-up of scripts/iss_bench.py), at the three radii of scripts/fpfh_ball_bench.py (about 31 / 100 / 300 other rows a ball).

(a) the grid build, the forward, the records pass, the gather, the whole forward + backward through autograd, and the rows VISITED per
    point by the forward's two walks and by the gather's one (the optional diagnostic counters, read in calls of their own that are not
    timed);
(b) iss_saliency_ball's pass (dicp_iss_ball_saliency) at the same radius on the same grid: the same two walks, the forward's yardstick;
(c) at the smallest radius, estimate_normals(k=32, method="grid") forward and forward + backward with both backward forms.
Every time is the median of --reps calls after one warm-up call, each between two HIP events.  Every line is printed, slower ones included.
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/normals_ball_bench.py [--clouds 256] [--points 16384] [--reps 5]
-> profiles/r37_normals_ball_bench.txt"""
import argparse
import json
import os

import torch

from dicp_amd import _lib
from dicp_amd._ops import _DT, _p, _workspace
from dicp_amd.iss import _ball_grid
from dicp_amd.normals import REC, estimate_normals, estimate_normals_ball

from iss_bench import G21, G32, MIN_NB, clouds, radius_for, timed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--members", default="31,100,300")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r37_normals_ball_bench.txt"))
    a = ap.parse_args()
    N, m = a.clouds, a.points
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
            dev, dt = P.device, _DT[dtype]
            g = torch.Generator(device="cpu").manual_seed(5)
            gn = torch.randn((N, m, 3), generator=g, dtype=dtype).to(dev)
            gk = torch.randn((N, m), generator=g, dtype=dtype).to(dev)
            ws_bytes = lib.dicp_normals_ball_workspace_bytes(N, m)
            ws = _workspace(ws_bytes, dev)
            iss_bytes = lib.dicp_iss_workspace_bytes(N, m)
            iss_ws = _workspace(iss_bytes, dev)
            nrm = torch.empty((N, m, 3), dtype=dtype, device=dev)
            curv = torch.empty((N, m), dtype=dtype, device=dev)
            sal = torch.empty((N, m), dtype=dtype, device=dev)
            grad = torch.empty((N, m, 3), dtype=dtype, device=dev)
            for members in [int(v) for v in a.members.split(",")]:
                radius = radius_for(layout, m, members + 1)                 # (radius_for counts the row itself)
                grid = _ball_grid(P, None, radius)
                gr = (_p(grid.plans), _p(grid.keys), _p(grid.perm), _p(grid.rows4))
                rec = torch.empty((N, grid.slots, REC), dtype=torch.float64, device=dev)
                visited = torch.zeros((2, N), dtype=torch.int64, device=dev)
                cnt = torch.empty((N, m), dtype=torch.int32, device=dev)

                def forward(v=None, c=None):
                    _lib.call("dicp_normals_ball_forward", dev, dt, *gr, N, m, radius, 3, None, 0, _p(ws), ws_bytes, _p(nrm), _p(curv), None, _p(c), _p(v))

                def records():
                    _lib.call("dicp_normals_ball_records", dev, dt, gr[0], gr[2], gr[3], N, m, _p(gn), _p(gk), _p(ws), ws_bytes, _p(rec))

                def gather(v=None):
                    _lib.call("dicp_normals_ball_gather", dev, dt, *gr, N, m, 3, radius, _p(rec), _p(grad), _p(v))

                def iss_pass():
                    _lib.call("dicp_iss_ball_saliency", dev, dt, *gr, N, m, radius, G21, G32, MIN_NB, _p(iss_ws), iss_bytes, _p(sal), None, None, None)

                def whole(backward):
                    x = P.detach().requires_grad_(backward)
                    n_, c_ = estimate_normals_ball(x, radius, return_curvature=True)
                    if backward:
                        torch.autograd.grad([n_, c_], [x], [gn, gk])

                def k_slot(backward, det):
                    x = P.detach().requires_grad_(backward)
                    n_, c_ = estimate_normals(x, k=K, return_curvature=True, method="grid", deterministic=det)
                    if backward:
                        torch.autograd.grad([n_, c_], [x], [gn, gk])
                forward(visited[0], cnt)                                    # the diagnostics, in calls of their own
                records()
                gather(visited[1])
                torch.cuda.synchronize()
                on = rec[..., 12] != 0
                row = {"layout": layout, "dtype": str(dtype).replace("torch.", ""), "B": N, "m": m, "members_asked": members,
                       "radius": round(radius, 5), "members_per_point": round(float(cnt.float().mean().item()) - 1.0, 1),
                       "members_max": int(cnt.max().item()) - 1,
                       "rows_visited_per_point_forward_two_walks": round(float(visited[0].sum().item()) / (N * m), 1),
                       "rows_visited_per_point_gather": round(float(visited[1].sum().item()) / (N * m), 1),
                       "rows_with_a_record_share": round(float(on.float().mean().item()) * grid.slots / m, 4)}
                row["grid_build_ms"] = round(timed(lambda: _ball_grid(P, None, radius), a.reps), 3)
                row["forward_ms"] = round(timed(forward, a.reps), 3)
                row["records_ms"] = round(timed(records, a.reps), 3)
                row["gather_ms"] = round(timed(gather, a.reps), 3)
                row["iss_ball_saliency_ms"] = round(timed(iss_pass, a.reps), 3)
                row["estimate_normals_ball_forward_ms"] = round(timed(lambda: whole(False), a.reps), 3)
                row["estimate_normals_ball_forward_backward_ms"] = round(timed(lambda: whole(True), a.reps), 3)
                row["forward_vs_iss_pass"] = round(row["forward_ms"] / row["iss_ball_saliency_ms"], 2)
                row["gather_vs_one_walk_of_the_iss_pass"] = round(row["gather_ms"] / (0.5 * row["iss_ball_saliency_ms"]), 2)
                row["gather_ns_per_member"] = round(row["gather_ms"] * 1e6 / (float(cnt.float().sum().item())), 3)
                if members <= K - 1:                                        # the radius at which the k-slot form holds about the same rows
                    row["k_slot_k32_grid_forward_ms"] = round(timed(lambda: k_slot(False, False), a.reps), 3)
                    row["k_slot_k32_grid_forward_backward_atomics_ms"] = round(timed(lambda: k_slot(True, False), a.reps), 3)
                    row["k_slot_k32_grid_forward_backward_deterministic_ms"] = round(timed(lambda: k_slot(True, True), a.reps), 3)
                    row["forward_vs_k_slot"] = round(row["estimate_normals_ball_forward_ms"] / row["k_slot_k32_grid_forward_ms"], 2)
                    row["forward_backward_vs_k_slot_deterministic"] = round(row["estimate_normals_ball_forward_backward_ms"]
                                                                            / row["k_slot_k32_grid_forward_backward_deterministic_ms"], 2)
                emit(row)
                del grid, rec, visited, cnt
            del P, ws, iss_ws, nrm, curv, sal, grad, gn, gk
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
