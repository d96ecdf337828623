"""Whole-ball FPFH (fpfh_features_ball: dicp_fpfh_ball_pack / _spfh / _combine on the cloud's cell grid) against the k-slot path
compute_fpfh(k=32) (ball_query -> dicp_fpfh_spfh -> dicp_fpfh_combine), in the same run on the same clouds: B = 256 x 16384 points, a
uniform volume and a planar scene, float32 and float64 (the set-up of scripts/fpfh_bench.py).

(a) at the radius whose ball holds about 31 other rows: the whole call of each form (not the same descriptor there: the k-slot form
    truncates the balls that hold more than 31 rows, and their share is printed);
(b) at the radii holding about 100 and about 300 rows, where only the whole-ball form is exact: the grid build, the pack, pass 1 and
    pass 2 on their own, and the rows VISITED per point by each pass (the optional diagnostic counters of the two entry points, read in
    a call of their own that is not timed);
(c) pass 2 with at = the whole-ball ISS keypoints of each cloud (compute_iss_keypoints at the 31-row radius, the index cut to the
    largest keypoint count) against pass 2 on every row.
Every time is the median of --reps calls after one warm-up call, each between two HIP events.
Run on an MI355X from the repo root: PYTHONPATH=. python scripts/fpfh_ball_bench.py [--clouds 256] [--points 16384] [--reps 5]
-> profiles/r36_fpfh_ball_bench.txt"""
import argparse
import json
import os

import torch

from dicp_amd import _lib
from dicp_amd._ops import _DT, _p, _workspace
from dicp_amd.fpfh import compute_fpfh, fpfh_features_ball
from dicp_amd.iss import _ball_grid, compute_iss_keypoints

from fpfh_bench import clouds, radius_for, timed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--members", default="31,100,300")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r36_fpfh_ball_bench.txt"))
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
            P, Nn = clouds(layout, N, m, dtype)
            dev, dt = P.device, _DT[dtype]
            ws_bytes = lib.dicp_fpfh_ball_workspace_bytes(dt, N, m)
            ws = _workspace(ws_bytes, dev)
            out = torch.empty((N, m, 33), dtype=dtype, device=dev)
            r_kp = radius_for(layout, m, K)
            _, kp_rows, index = compute_iss_keypoints(P, r_kp, whole_ball=True, return_index=True)
            q = max(int(kp_rows.max().item()), 1)
            at = index[:, :q].contiguous()
            out_at = torch.empty((N, q, 33), dtype=dtype, device=dev)
            for members in [int(v) for v in a.members.split(",")]:
                radius = radius_for(layout, m, members + 1)                 # (radius_for counts the row itself)
                grid = _ball_grid(P, None, radius)
                g = (_p(grid.plans), _p(grid.keys), _p(grid.perm), _p(grid.rows4))
                visited = torch.zeros((3, N), dtype=torch.int64, device=dev)
                spfh = torch.empty((N, m, 33), dtype=torch.int32, device=dev)

                def pack():
                    _lib.call("dicp_fpfh_ball_pack", dev, dt, g[0], g[2], g[3], _p(Nn), N, m, _p(ws), ws_bytes)

                def pass1(v=None, s=None):
                    _lib.call("dicp_fpfh_ball_spfh", dev, dt, *g, N, m, radius, _p(ws), ws_bytes, _p(s), _p(v))

                def pass2(v=None):
                    _lib.call("dicp_fpfh_ball_combine", dev, dt, *g, None, 0, 0, N, m, radius, _p(ws), ws_bytes, _p(out), _p(v))

                def pass2_at(v=None):
                    _lib.call("dicp_fpfh_ball_combine", dev, dt, *g, _p(at), 1, q, N, m, radius, _p(ws), ws_bytes, _p(out_at), _p(v))
                pack()
                pass1(visited[0], spfh)                                     # the diagnostics, in calls of their own
                pass2(visited[1])
                pass2_at(visited[2])
                torch.cuda.synchronize()
                pairs = spfh[..., :11].sum(-1)
                row = {"layout": layout, "dtype": str(dtype).replace("torch.", ""), "B": N, "m": m, "members_asked": members,
                       "radius": round(radius, 5), "pairs_per_point": round(float(pairs.float().mean().item()), 1), "pairs_max": int(pairs.max().item()),
                       "rows_visited_per_point_pass1": round(float(visited[0].sum().item()) / (N * m), 1),
                       "rows_visited_per_point_pass2": round(float(visited[1].sum().item()) / (N * m), 1),
                       "keypoints_per_cloud": round(float(kp_rows.float().mean().item()), 1), "at_entries_per_cloud": q,
                       "rows_visited_per_keypoint_pass2_at": round(float(visited[2].sum().item()) / max(int(kp_rows.sum().item()), 1), 1),
                       "workspace_MB": round(ws_bytes / 2 ** 20, 1)}
                row["grid_build_ms"] = round(timed(lambda: _ball_grid(P, None, radius), a.reps), 3)
                row["pack_ms"] = round(timed(pack, a.reps), 3)
                row["pass1_spfh_ms"] = round(timed(pass1, a.reps), 3)
                row["pass2_combine_ms"] = round(timed(pass2, a.reps), 3)
                row["pass2_at_keypoints_ms"] = round(timed(pass2_at, a.reps), 3)
                row["pass2_all_over_at"] = round(row["pass2_combine_ms"] / row["pass2_at_keypoints_ms"], 1)
                row["fpfh_features_ball_ms"] = round(timed(lambda: fpfh_features_ball(P, Nn, radius), a.reps), 3)
                row["fpfh_features_ball_at_keypoints_ms"] = round(timed(lambda: fpfh_features_ball(P, Nn, radius, at=at), a.reps), 3)
                row["ns_per_point_and_visited_row_pass1"] = round(row["pass1_spfh_ms"] * 1e6 / (visited[0].sum().item()), 4)
                row["ns_per_point_and_visited_row_pass2"] = round(row["pass2_combine_ms"] * 1e6 / (visited[1].sum().item()), 4)
                if members <= K - 1:                                        # the radius at which the k-slot path is meant to be used
                    t_k = timed(lambda: compute_fpfh(P, Nn, radius, k=K), a.reps)
                    row.update({"k_slot_compute_fpfh_k32_ms": round(t_k, 3), "whole_call_speedup": round(t_k / row["fpfh_features_ball_ms"], 2),
                                "rows_beyond_32_slots_share": round(float((pairs > K - 1).float().mean().item()), 4)})
                emit(row)
                del grid, visited, spfh
            del P, Nn, ws, out, out_at, at, index
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
