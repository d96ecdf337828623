"""Wall time per call of each point-cloud operator on one 256-row float32 cloud already on the device: median of 200 calls after 20
warm-up calls, each call timed to the end of its GPU work (synchronize).  The tree under test comes from PYTHONPATH."""
import json
import statistics
import sys
import time

import torch

import dicp_amd
from dicp_amd.ball import ball_query
from dicp_amd.fps import sample_farthest_points
from dicp_amd.group import group_points, interpolate_features, pool_neighbors
from dicp_amd.knn import chamfer_distance, knn_points
from dicp_amd.normals import estimate_normals
from dicp_amd.voxel import voxel_downsample

g = torch.Generator().manual_seed(3)
x = torch.rand(256, 3, generator=g).cuda()
y = torch.rand(256, 3, generator=g).cuda()
f = torch.rand(256, 64, generator=g).cuda()                # C = 64 features on the rows of y, gathered through k = 16 neighbours
d2, idx = knn_points(x, y, k=16)
OPS = {
    "estimate_normals": lambda: estimate_normals(x, k=16),
    "voxel_downsample": lambda: voxel_downsample(x, 0.1),
    "knn_points": lambda: knn_points(x, y, k=8),
    "chamfer_distance": lambda: chamfer_distance(x, y),
    "sample_farthest_points": lambda: sample_farthest_points(x, 64),
    "ball_query": lambda: ball_query(x, y, 0.2, k=16),
    "knn_points_grid": lambda: knn_points(x, y, k=8, method="grid"),
    "group_points": lambda: group_points(f, idx),
    "pool_neighbors": lambda: pool_neighbors(f, idx),
    "interpolate_features": lambda: interpolate_features(f, idx, d2),
}
rec = {"tree": dicp_amd.__file__, "label": sys.argv[1] if len(sys.argv) > 1 else ""}
for name, fn in OPS.items():
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(200):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    rec[name + "_us"] = round(statistics.median(ts), 1)
print(json.dumps(rec), flush=True)
