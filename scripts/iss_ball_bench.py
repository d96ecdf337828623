"""Whole-ball ISS keypoints (iss_keypoints_ball: dicp_iss_ball_saliency / dicp_iss_ball_maxima on the cloud's cell grid) against the k-slot
path compute_iss_keypoints(k=32) (ball_query -> dicp_iss_saliency -> dicp_iss_maxima), in the same run on the same clouds: B = 256 x 16384
points, a uniform volume and a planar scene, float32 and float64 (the set-up of scripts/iss_bench.py).

(a) at the radius whose ball holds about 31 other rows -- the same members in both forms, like for like: the whole call, and each pass of
    the whole-ball form against ball_query + the k-slot pass;
(b) at the radii holding about 100 and about 300 rows, where only the whole-ball form is exact: its times and the rows VISITED per point
    (the optional diagnostic counters of the two entry points, read in a call of their own that is not timed);
(c) the grid build alone (CellGrid at the call's radius).
Every time is the median of --reps calls after one warm-up call, each between two HIP events.
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/iss_ball_bench.py [--clouds 256] [--points 16384] [--reps 5]
-> profiles/r35_iss_ball_bench.txt"""
import argparse
import json
import os

import torch

from dicp_amd import _lib
from dicp_amd._ops import _DT, _p, _workspace
from dicp_amd.ball import ball_query
from dicp_amd.iss import _ball_grid, compute_iss_keypoints, iss_keypoints_ball

from iss_bench import G21, G32, MIN_NB, clouds, radius_for, timed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--members", default="31,100,300")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r35_iss_ball_bench.txt"))
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
            dt = _DT[dtype]
            ws_bytes = lib.dicp_iss_workspace_bytes(N, m)
            ws = _workspace(ws_bytes, P.device)
            sal = torch.empty((N, m), dtype=dtype, device=P.device)
            mask = torch.empty((N, m), dtype=torch.bool, device=P.device)
            for members in [int(v) for v in a.members.split(",")]:
                radius = radius_for(layout, m, members + 1)                 # (radius_for counts the row itself)
                grid = _ball_grid(P, None, radius)
                visited = torch.zeros((2, N), dtype=torch.int64, device=P.device)
                cnt = torch.empty((N, m), dtype=torch.int32, device=P.device)

                def ball1(v=None, c=None):
                    _lib.call("dicp_iss_ball_saliency", P.device, dt, _p(grid.plans), _p(grid.keys), _p(grid.perm), _p(grid.rows4), N, m, radius,
                              G21, G32, MIN_NB, _p(ws), ws_bytes, _p(sal), None, _p(c), _p(v))

                def ball2(v=None):
                    _lib.call("dicp_iss_ball_maxima", P.device, dt, _p(grid.plans), _p(grid.keys), _p(grid.perm), _p(grid.rows4), N, m, radius,
                              MIN_NB, _p(ws), ws_bytes, _p(mask), _p(v))
                ball1(visited[0], cnt)                                      # the diagnostics, in calls of their own
                ball2(visited[1])
                torch.cuda.synchronize()
                row = {"layout": layout, "dtype": str(dtype).replace("torch.", ""), "B": N, "m": m, "members_asked": members,
                       "radius": round(radius, 5), "members_per_point": round(float(cnt.float().mean().item()) - 1.0, 1),
                       "members_max": int(cnt.max().item()) - 1,
                       "rows_visited_per_point_saliency_two_walks": round(float(visited[0].sum().item()) / (N * m), 1),
                       "rows_visited_per_point_maxima": round(float(visited[1].sum().item()) / (N * m), 1),
                       "salient_share": round(float((sal > 0).float().mean().item()), 4)}
                row["grid_build_ms"] = round(timed(lambda: _ball_grid(P, None, radius), a.reps), 3)
                row["ball_saliency_ms"] = round(timed(ball1, a.reps), 3)
                row["ball_maxima_ms"] = round(timed(ball2, a.reps), 3)
                row["iss_keypoints_ball_ms"] = round(timed(lambda: iss_keypoints_ball(P, radius), a.reps), 3)
                row["compute_whole_ball_ms"] = round(timed(lambda: compute_iss_keypoints(P, radius, whole_ball=True), a.reps), 3)
                row["keypoints_per_cloud_whole_ball"] = round(float(mask.sum().item()) / N, 1)
                if members <= K - 1:                                        # like for like: the k-slot path holds the same members
                    idx = ball_query(P, P, radius, k=K)[1]
                    mask_k = torch.empty((N, m), dtype=torch.bool, device=P.device)

                    def slot1():
                        _lib.call("dicp_iss_saliency", P.device, dt, _p(P), 3, _p(idx), 1, None, N, m, K, radius, G21, G32, MIN_NB, _p(ws), ws_bytes,
                                  _p(sal), None, None)

                    def slot2():
                        _lib.call("dicp_iss_maxima", P.device, dt, _p(P), 3, _p(idx), 1, None, N, m, K, radius, MIN_NB, _p(ws), ws_bytes, _p(mask_k))
                    t_ball = timed(lambda: ball_query(P, P, radius, k=K), a.reps)
                    t1, t2 = timed(slot1, a.reps), timed(slot2, a.reps)
                    row.update({"k_slot_ball_query_ms": round(t_ball, 3), "k_slot_saliency_ms": round(t1, 3), "k_slot_maxima_ms": round(t2, 3),
                                "k_slot_compute_k32_ms": round(timed(lambda: compute_iss_keypoints(P, radius, k=K), a.reps), 3),
                                "k_slot_slots_filled": round(float((idx >= 0).float().mean().item()), 3),
                                "k_slot_rows_truncated_share": round(float((cnt > K).float().mean().item()), 4),
                                "masks_equal_share": round(float((mask_k == mask).float().mean().item()), 5)})
                    row["whole_call_speedup"] = round(row["k_slot_compute_k32_ms"] / row["compute_whole_ball_ms"], 2)
                    row["saliency_vs_query_plus_pass"] = round((t_ball + t1) / (row["grid_build_ms"] + row["ball_saliency_ms"]), 2)
                    row["maxima_vs_query_plus_pass"] = round((t_ball + t2) / (row["grid_build_ms"] + row["ball_maxima_ms"]), 2)
                    del idx, mask_k
                emit(row)
                del grid, visited, cnt
            del P, ws, sal, mask
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
