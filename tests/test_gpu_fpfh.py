"""fpfh_features / compute_fpfh on the MI355X (dicp_amd/fpfh.py; csrc/fpfh.hip) against the numpy restatement tests/fpfh_ref.py: the bin
counts of pass 1 integer for integer, the descriptor bit for bit.

1  shapes at the edges of the kernels' tiles: m in {1, 2, 63, 64, 65, 300, 1500} x k in {1, 2, 3, 7, 8, 31, 32}, float32 and float64, int64
   and int32 indices, two clouds of different row counts per call, dead rows and garbage indices in every cloud;
2  ragged batches with a cloud of no rows, pad rows holding NaN and slots of every kind; extra point columns holding NaN;
3  the designed clouds of tests/fpfh_cases.py (a pair at the centre of every bin, the clamp, theta = pi with either zero, the tie, d parallel
   to n1, duplicates, dead normals, the row itself, garbage indices);
4  an idx straight from ball_query, from knn_points(method="grid") cut by radius=, and a hand-made one between guard regions;
5  single clouds, lists and CPU tensors against the batch; no gradient;  6  a call in a captured graph;
7  end to end on a structured scene: normals -> compute_fpfh -> match_features -> ransac_correspondences -> ICP recovers a pose that ICP
   alone does not.
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.ball import ball_query
from dicp_amd.fpfh import compute_fpfh, fpfh_features
from dicp_amd.ICP import ICP
from dicp_amd.knn import knn_points
from dicp_amd.match import match_features, ransac_correspondences
from dicp_amd.normals import estimate_normals

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_cases as fc  # noqa: E402
import fpfh_ref as fr  # noqa: E402
from ransac_ref import rotation_error  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
M_CASES = (1, 2, 63, 64, 65, 300, 1500)
K_CASES = (1, 2, 3, 7, 8, 31, 32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check(P, Nn, idx, rows, radius=None, itype=np.int64, ref=None):
    """one batched call against the reference (computed here unless given) -> the reference"""
    idx_t = fc.index_dtype(idx, itype)
    ref = fr.fpfh_ref_batch(P, Nn, idx_t, rows, radius) if ref is None else ref
    rows_t = None if rows is None else torch.tensor(np.asarray(rows), dtype=torch.int32).cuda()
    out, spfh = fpfh_features(dev(P), dev(Nn), dev(idx_t), rows=rows_t, radius=radius, return_spfh=True)
    assert out.shape == P.shape[:2] + (33,) and spfh.shape == out.shape and spfh.dtype == torch.uint8 and spfh.is_contiguous()
    assert out.dtype == dev(P).dtype and not out.requires_grad
    assert np.array_equal(host(spfh), ref[1])
    assert fr.same_bits(host(out), ref[0])
    return ref


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", M_CASES)
def test_tile_edges(dtype, m):
    for q, k in enumerate(K_CASES):
        a = fc.random_cloud(100 * m + k, m, k, dtype)
        b = fc.random_cloud(100 * m + k + 50, m, k, dtype, rows=m - m // 3, planar=True)
        P, Nn, idx, rows = fc.pad_batch([a, b])
        radius = (None, 0.5, 0.2)[q % 3] if m >= 63 else None
        ref = check(P, Nn, idx, rows, radius, itype=(np.int64, np.int32)[q % 2])
        if m >= 300 and k >= 7:
            assert ref[1].sum() > m                                 # (the case is not empty)
        if m == 300 and k in (8, 31):
            check(P, Nn, idx, rows, radius, itype=(np.int32, np.int64)[q % 2], ref=ref)


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_batch_with_an_empty_cloud(dtype):
    rows = [300, 0, 157, 64, 1]
    clouds = [fc.random_cloud(7 + b, 300, 16, dtype, rows=r, cols=5, planar=(b == 2)) for b, r in enumerate(rows)]
    P, Nn, idx, rw = fc.pad_batch(clouds)
    assert np.isnan(P[..., 3:]).all() and np.isnan(P[1]).all()
    ref = check(P, Nn, idx, rw, 0.4)
    assert not ref[0][1].any() and not ref[0][4].any() and ref[1][0].sum() > 0
    check(P, Nn, idx, None, ref=fr.fpfh_ref_batch(P, Nn, idx, None))  # no rows: the NaN rows are dead all the same


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("dtype", DTYPES)
def test_designed_clouds(dtype):
    d = fc.designed(dtype)
    P, Nn, idx, rows = fc.pad_batch(list(d.values()))
    ref = check(P, Nn, idx, rows)
    check(P, Nn, idx, rows, itype=np.int32, ref=ref)
    names = list(d)
    cnt = ref[1]
    bc = cnt[names.index("bin_centres")]
    assert all(bc[2 * p, p] == 1 and bc[2 * p + 1, p] == 1 for p in range(33))
    assert (cnt[names.index("theta_pi")][:32, :11].argmax(axis=1) == 10).all()
    assert list(np.flatnonzero(cnt[names.index("tie")][0])) == [8, 16, 30]
    assert list(cnt[names.index("parallel")][:3].sum(axis=1)) == [0, 3, 3]


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("dtype", DTYPES)
def test_idx_of_the_searches(dtype):
    clouds = [fc.random_cloud(31 + b, 700, 1, dtype, rows=r, garbage=False) for b, r in enumerate((700, 520))]
    P, Nn, _, rows = fc.pad_batch(clouds)
    Pd, Nd, rw = dev(P), dev(Nn), torch.tensor(rows).cuda()
    radius = 0.3
    _, idx_ball = ball_query(Pd, Pd, radius, k=24, x_rows=rw, y_rows=rw)
    _, idx_knn = knn_points(Pd, Pd, 24, x_rows=rw, y_rows=rw, method="grid")
    assert (idx_ball >= 0).sum() > 3 * 700 and (idx_ball == -1).any()
    ref = check(P, Nn, host(idx_ball), rows, radius)
    got = compute_fpfh(Pd, Nd, radius, k=24, rows=rw)
    assert fr.same_bits(host(got), ref[0])
    hybrid = check(P, Nn, host(idx_knn), rows, radius)              # the k nearest, cut by the recomputed distance: the same neighbours
    if dtype == np.float64:                                         # (float32: the search's own d2 decides at the rim of the ball)
        assert np.array_equal(hybrid[1], ref[1])
    check(P, Nn, host(idx_knn), rows)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("itype", [torch.int64, torch.int32])
def test_hand_made_idx_between_guard_regions(dtype, itype):
    N, m, k, G = 2, 130, 9, 4096
    rows = [130, 77]
    rng = np.random.default_rng(5)
    clouds = [fc.random_cloud(41 + b, m, k, dtype, rows=r) for b, r in enumerate(rows)]
    P, Nn, idx, rw = fc.pad_batch(clouds)
    idx[:, ::7, 0], idx[:, 1::7, 2], idx[:, 2::7, 4], idx[:, 3::7, 5] = -1, -7, 77, 130       # (77 = rows of cloud 1, 130 = m)
    idx[:, 4::7, 6] = rng.integers(131, 1 << 30, idx[:, 4::7, 6].shape)
    idx = fc.index_dtype(idx, np.int32 if itype == torch.int32 else np.int64)
    ref = fr.fpfh_ref_batch(P, Nn, idx, rw)

    def guarded(a, fill, dt):
        big = torch.full((a.size + 2 * G,), fill, dtype=dt).cuda()
        big[G:G + a.size] = dev(a).reshape(-1).to(dt)
        return big, big[G:G + a.size].view(a.shape)
    fdt = torch.float32 if dtype == np.float32 else torch.float64
    bp, Pg = guarded(P, float("nan"), fdt)
    bn, Ng = guarded(Nn, float("nan"), fdt)
    bi, Ig = guarded(idx, 3, itype)                                 # (a guard that would name a live row if it were read)
    out, spfh = fpfh_features(Pg, Ng, Ig, rows=torch.tensor(rw).cuda(), return_spfh=True)
    assert np.array_equal(host(spfh), ref[1]) and fr.same_bits(host(out), ref[0])
    for big, a in ((bp, P), (bn, Nn)):                              # (the inputs are read only: the guards are as they were)
        assert bool(torch.isnan(big[:G]).all()) and bool(torch.isnan(big[G + a.size:]).all())
    assert bool((bi[:G] == 3).all()) and bool((bi[G + idx.size:] == 3).all())


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("dtype", DTYPES)
def test_forms(dtype):
    rows = [90, 61, 75]
    clouds = [fc.random_cloud(51 + b, 90, 12, dtype, rows=r) for b, r in enumerate(rows)]
    P, Nn, idx, rw = fc.pad_batch(clouds)
    ref = check(P, Nn, idx, rw, 0.6)
    for b, r in enumerate(rows):
        out, spfh = fpfh_features(dev(P[b, :r]), dev(Nn[b, :r]), dev(idx[b, :r]), radius=0.6, return_spfh=True)
        assert out.shape == (r, 33) and fr.same_bits(host(out), ref[0][b, :r]) and np.array_equal(host(spfh), ref[1][b, :r])
    lists = [[dev(a[b, :r]) for b, r in enumerate(rows)] for a in (P, Nn, idx)]
    outs = fpfh_features(*lists, radius=0.6)
    assert isinstance(outs, list) and all(fr.same_bits(host(o), ref[0][b, :r]) for b, (o, r) in enumerate(zip(outs, rows)))
    on_cpu = fpfh_features(torch.from_numpy(P), torch.from_numpy(Nn), torch.from_numpy(idx), rows=torch.tensor(rows), radius=0.6)
    assert not on_cpu.is_cuda and fr.same_bits(on_cpu.numpy(), ref[0])
    x = dev(P[0]).requires_grad_(True)
    n = dev(Nn[0]).requires_grad_(True)
    out = fpfh_features(x, n, dev(idx[0]), radius=0.6)
    assert not out.requires_grad and fr.same_bits(host(out), ref[0][0])
    lists_c = compute_fpfh([t[..., :3] for t in lists[0]], lists[1], 0.6, k=12)
    batch_c = compute_fpfh(dev(P), dev(Nn), 0.6, k=12, rows=torch.tensor(rows).cuda())
    assert all(fr.same_bits(host(o), host(batch_c[b, :r])) for b, (o, r) in enumerate(zip(lists_c, rows)))


# ------------------------------------------------------------------ 6
def test_captured_call():
    rows = [400, 333]

    def data(seed):
        clouds = [fc.random_cloud(seed + b, 400, 16, np.float32, rows=r) for b, r in enumerate(rows)]
        P, Nn, idx, rw = fc.pad_batch(clouds)
        return {"P": dev(P), "N": dev(Nn), "idx": dev(idx), "rows": torch.tensor(rw, dtype=torch.int32).cuda()}

    def run(s):
        return fpfh_features(s["P"], s["N"], s["idx"], rows=s["rows"], radius=0.5, return_spfh=True)
    static = data(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(static)
    for seed in (20, 30):
        fresh = data(seed)
        for key, t in fresh.items():
            static[key].copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(fresh)
        torch.cuda.synchronize()
        assert fr.same_bits(host(captured[0]), host(eager[0])) and torch.equal(captured[1], eager[1])
        assert captured[1].sum() > 0


# ------------------------------------------------------------------ 7
E2E_CPU_SHARE = 0.508             # profiles/r27_fpfh_edges.txt: the share that tests/fpfh_ref.py alone reaches on this scene, on the CPU


def test_end_to_end_registration():
    """The chain of the README on the seeded scene of tests/fpfh_cases.py: m = 1500, the source an 85 % subset, rotated by 1 rad about a nearly
    vertical axis (a vehicle's turn: ICP alone is trapped), moved metres away, 2 mm of noise.  scripts/fpfh_edges.py measured the share of mutual matches within 0.15 of the true row with tests/fpfh_ref.py
    alone, on the CPU, before any threshold here was fixed (profiles/r27_fpfh_edges.txt): E2E_CPU_SHARE; the GPU run must reach half of it."""
    P = fc.scene(0, 1500)
    mv = fc.moved_copy(P, seed=0, keep=0.85, angle=1.0, noise=0.002, axis=fc.E2E_AXIS)
    y, x = dev(P.astype(np.float32)), dev(mv["x"].astype(np.float32))
    vp_y = torch.tensor(fc.VIEWPOINT, dtype=torch.float32)
    vp_x = torch.tensor(fc.VIEWPOINT @ mv["R"].T + mv["t"], dtype=torch.float32)
    ny = estimate_normals(y, k=16, viewpoint=vp_y)
    nx = estimate_normals(x, k=16, viewpoint=vp_x)
    fx, fy = compute_fpfh(x, nx, 0.8, k=32), compute_fpfh(y, ny, 0.8, k=32)
    idx, _ = match_features(fx, fy, mutual=True)
    got = host(idx)
    live = got >= 0
    err = np.linalg.norm(P[np.where(live, got, 0)] - P[mv["src"]], axis=1)
    share = float((err[live] <= 0.15).mean())
    print("mutual matches %d of %d, within 0.15 of the true row: %.3f (CPU reference: %.3f)" % (live.sum(), live.size, share, E2E_CPU_SHARE))
    assert live.sum() >= 100 and share >= 0.5 * E2E_CPU_SHARE
    thr = 0.15
    T0, inl = ransac_correspondences(x, y, idx, thr, hypotheses=4096, seed=7, refine=2)
    C_true, r_true = mv["R"].T, -mv["R"].T @ mv["t"]
    T0h = host(T0).astype(np.float64)
    moved = mv["x"] @ T0h[:3, :3].T + T0h[:3, 3]
    worst = float(np.linalg.norm(moved - P[mv["src"]], axis=1).max())
    print("RANSAC: %d inliers; the worst true pair is %.4f apart under its pose (threshold %.2f)" % (int(inl.sum()), worst, thr))
    assert worst <= thr
    icp = ICP(icp_type="pt2pt", max_iterations=30, tolerance=1e-9)
    err = {}
    for name, Ti in (("ransac", T0), ("identity", torch.eye(4, dtype=torch.float32).cuda())):
        out = icp.icp(x[None], y[None], T_init=Ti[None])
        Th = host(out["T"][0]).astype(np.float64)
        err[name] = (rotation_error(Th[:3, :3].reshape(-1), C_true), float(np.linalg.norm(Th[:3, 3] - r_true)))
    print("ICP from the RANSAC pose: %.3g rad, %.3g m; from the identity: %.3g rad, %.3g m" % (err["ransac"] + err["identity"]))
    assert err["ransac"][0] < 1e-2 and err["ransac"][1] < 5e-2
    assert err["identity"][0] > 0.5                                 # the reason the descriptor exists

