"""knn_points / chamfer_distance with method="grid" on the MI355X against their definition: index for index and d2 bit for bit against the
numpy brute force walk_layouts.knn_oracle AND against method="walk" -- random cubes, the lattice's ties across cells, degenerate layouts
(one cell, lines, a wall, clusters, far queries, k above the row count, the flat plan), non-finite and ragged rows, every input form, the
layouts of the walk's out-of-window tests; against ball_query inside a radius; the rows-visited counters against the host build of the same
header; the gradients within the derived bounds of walk_layouts.knn_grad_check; reproducibility; no host synchronisation; graph capture."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.ball import ball_query
from dicp_amd.knn import chamfer_distance, knn_points
from dicp_amd.synthetic import make_pairs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ball_clouds as bc  # noqa: E402
import gridknn_host as gh  # noqa: E402
import walk_layouts as wl  # noqa: E402
from ball_ref import r2_of  # noqa: E402
from test_gpu_knn_walk import _case as _walk_case  # noqa: E402  (the layouts' brute force, computed once per process for both files)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
KMAX = max(gh.KS)


def _np(outs):
    return tuple(o.detach().cpu().numpy() for o in outs)


def _hold(x, y, ks=gh.KS, ref=None):
    """one pair of clouds on the device at every k: the grid against the brute force at the largest k, and against the walk"""
    ref = ref if ref is not None else gh.reference(x, y, max(ks))
    xd, yd = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(y)).cuda()
    for k in ks:
        d2, idx = knn_points(xd, yd, k=k, method="grid")
        assert d2.shape == (x.shape[0], k) and idx.shape == (x.shape[0], k) and d2.dtype == xd.dtype and idx.dtype == torch.int64
        bad = gh.same(_np((d2, idx)), (ref[0][:, :k], ref[1][:, :k]))
        assert bad is None, "k=%d against the brute force: %s" % (k, bad)
        bad = gh.same(_np((d2, idx)), _np(knn_points(xd, yd, k=k)))
        assert bad is None, "k=%d against the walk: %s" % (k, bad)
    return ref


@functools.lru_cache(maxsize=None)
def _random_ref(n, m, dtype):
    x, y = bc.random_pair(n, m, dtype)
    ref = gh.reference(x, y, KMAX)
    for a in (x, y) + ref:
        a.setflags(write=False)
    return x, y, ref


# ------------------------------------------------------------------ 1. the forward against the brute force and the walk
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", bc.RANDOM_SHAPES)
def test_random_cubes(n, m, dtype):
    x, y, ref = _random_ref(n, m, dtype)
    _hold(x, y, ref=ref)


def test_a_cloud_of_many_sort_chunks():
    """20000 rows: 32768 sorted slots, 16 LDS chunks and every stride of the sort between them"""
    x, y = bc.random_pair(300, 20000, np.float32)
    _hold(x, y, ks=(8,))


@pytest.mark.parametrize("dtype", DTYPES)
def test_lattice_degenerate_and_far_layouts(dtype):
    names = set()
    for name, x, y in gh.all_cases(dtype):
        ref = _hold(x, y)
        names.add(name)
        if name == "lattice r=1.0":
            assert ref[1][171, :7].tolist() == [171, 122, 164, 170, 172, 178, 220]         # six rows at d2 = 1 in six cells: by index
        if name == "k above the live rows":
            assert (ref[1][:, 4:] == -1).all() and (ref[1][:, :4] >= 0).all()
        if name == "queries at 1e30":
            assert (ref[1][:4] == -1).all() and (ref[1][4] >= 0).all()
    assert {"300 copies", "line along z", "line along x", "wall", "two clusters", "far queries", "small cluster facing a far one",
            "queries 1e6 extents away", "extent 3e38"} <= names
    assert ("queries at 1e30" in names) == (dtype == np.float32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_rows(dtype):
    x, y = bc.nonfinite_pair(dtype)
    ref = _hold(x, y)
    assert (ref[1][[0, 7, 150]] == -1).all() and not np.isin(ref[1], [5, 17, 400, 899]).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", wl.KNN_LAYOUTS)
def test_out_of_window_layouts(name, dtype):
    X, Y, k, d2o, io, _ = _walk_case(name, dtype)
    d2, idx = knn_points(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), k=k, method="grid")
    bad = gh.same(_np((d2, idx)), (d2o, io))
    assert bad is None, bad
    g = np.random.default_rng(7).standard_normal(io.shape).astype(X.dtype)
    x = torch.from_numpy(X).cuda().requires_grad_(True)
    y = torch.from_numpy(Y).cuda().requires_grad_(True)
    d2, idx = knn_points(x, y, k=k, method="grid")
    torch.autograd.backward(d2, torch.from_numpy(g).cuda())
    rx, ry = wl.knn_grad_check(X, Y, io, g, x.grad.cpu().numpy(), y.grad.cpu().numpy(), dtype, name)       # dense_queries: in-degree ~3000
    print("%s %s: worst error / bound: x-gradient %.3f, y-gradient %.3f" % (name, X.dtype.name, rx, ry))


# ------------------------------------------------------------------ 2. against ball_query, and the counters against the host build
@pytest.mark.parametrize("dtype", DTYPES)
def test_equals_ball_query_inside_the_radius(dtype):
    for (x, y), r in ((bc.random_pair(700, 5000, dtype), 0.1), (bc.wall_pair(400, 3000, dtype), 0.05)):
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        r2 = torch.tensor(r2_of(r, dtype)).cuda()
        for k in gh.KS:
            kd2, kidx = knn_points(xd, yd, k=k, method="grid")
            out = kd2 > r2
            kd2 = torch.where(out, torch.full_like(kd2, float("inf")), kd2)
            kidx = torch.where(out, torch.full_like(kidx, -1), kidx)
            d2, idx = ball_query(xd, yd, r, k=k)
            assert (~out).any() and (out.any() or k == 1)   # (at k = 1 every nearest row lies inside the radius)
            assert torch.equal(idx, kidx) and d2.cpu().numpy().tobytes() == kd2.cpu().numpy().tobytes()


def test_visited_counters_equal_the_host_build():
    """the same header on the host and on the device: the same plan (the edge bit for bit), the same cells, the same rows"""
    pairs = [bc.random_pair(700, 5000, np.float32), bc.random_pair(700, 5000, np.float32, seed=1)]
    X = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    Y = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    for k in (1, 8, 32):
        visited = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        passes = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        knn_points(X, Y, k=k, method="grid", _visited=visited, _passes=passes)
        for b, (x, y) in enumerate(pairs):
            _, st = gh.header(x, y, k)
            assert (int(visited[b]), int(passes[b])) == (st["visited"], st["passes"]), (k, b)


# ------------------------------------------------------------------ 3. ragged batches and input forms
@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_batches_and_input_forms(dtype):
    tdt = TORCH[dtype]
    k = 8
    sizes = ((300, 900), (120, 0), (0, 500), (257, 40), (1, 1), (50, 5))
    clouds = [bc.random_pair(max(n, 1), max(m, 1), dtype, seed=20 + i) for i, (n, m) in enumerate(sizes)]
    clouds = [(x[:n], y[:m]) for (x, y), (n, m) in zip(clouds, sizes)]
    clouds[0] = bc.nonfinite_pair(dtype)
    singles = [_np(knn_points(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), k=k, method="grid")) for x, y in clouds]
    for (x, y), s in zip(clouds, singles):
        assert gh.same(s, gh.reference(x, y, k)) is None
    N, n_max, m_max = len(sizes), 300, 900
    for fill in ("nan", "decoy"):                           # pad rows: NaN, and rows that would be neighbours if they took part
        X = np.full((N, n_max, 3), np.nan, dtype=dtype)
        Y = np.full((N, m_max, 3), np.nan, dtype=dtype)
        if fill == "decoy":
            X[:], Y[:] = 0.5, 0.5
            Y[:, :, 0] += np.linspace(0, 0.01, m_max, dtype=dtype)
        for b, (x, y) in enumerate(clouds):
            X[b, :x.shape[0]], Y[b, :y.shape[0]] = x, y
        xr = torch.tensor([s[0] for s in sizes], dtype=torch.int32)
        yr = torch.tensor([s[1] for s in sizes], dtype=torch.int64)
        for rows_dev in ("cuda", "cpu"):
            d2, idx = knn_points(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), k=k, x_rows=xr.to(rows_dev), y_rows=yr.to(rows_dev), method="grid")
            assert d2.shape == (N, n_max, k)
            d2, idx = _np((d2, idx))
            for b, (n, m) in enumerate(sizes):
                bad = gh.same((d2[b, :n], idx[b, :n]), singles[b])
                assert bad is None, "%s cloud %d: %s" % (fill, b, bad)
                assert np.isinf(d2[b, n:]).all() and (idx[b, n:] == -1).all()
    # lists
    ld2, lidx = knn_points([torch.from_numpy(x).cuda() for x, _ in clouds], [torch.from_numpy(y).cuda() for _, y in clouds], k=k, method="grid")
    for b, (n, m) in enumerate(sizes):
        assert ld2[b].shape == (n, k) and gh.same(_np((ld2[b], lidx[b])), singles[b]) is None
    # single clouds from the CPU, 6 columns, a non-contiguous view
    x, y = clouds[0]
    outs = knn_points(torch.from_numpy(x), torch.from_numpy(y), k=k, method="grid")
    assert all(o.device.type == "cpu" for o in outs) and outs[0].dtype == tdt and gh.same(_np(outs), singles[0]) is None
    x6 = torch.from_numpy(np.concatenate([x, x + 5], 1)).cuda()
    y6 = torch.from_numpy(np.concatenate([y, y - 5], 1)).cuda()
    assert gh.same(_np(knn_points(x6, y6, k=k, method="grid")), singles[0]) is None
    wide = torch.from_numpy(np.concatenate([y, y, y], 1)).cuda()[:, 3:7]
    assert not wide.is_contiguous()
    assert gh.same(_np(knn_points(torch.from_numpy(x).cuda(), wide, k=k, method="grid")), singles[0]) is None
    e = knn_points(torch.zeros((0, 3), dtype=tdt).cuda(), torch.from_numpy(y).cuda(), k=k, method="grid")
    assert e[0].shape == (0, k) and e[1].shape == (0, k)


# ------------------------------------------------------------------ 4. gradients
def test_gradcheck_float64():
    g = torch.Generator().manual_seed(3)
    x = torch.rand((40, 3), generator=g, dtype=torch.float64).cuda().requires_grad_(True)
    y = torch.rand((30, 3), generator=g, dtype=torch.float64).cuda().requires_grad_(True)
    for k in (1, 5):
        assert torch.autograd.gradcheck(lambda a, b: knn_points(a, b, k=k, method="grid")[0], (x, y), eps=1e-7, atol=1e-6)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_gradient_beyond_xyz_pad_rows_and_empty_slots_and_runs_repeat(dtype):
    """columns 3.., pad rows and -1 slots get exactly zero with NaN cotangents there; the forward and the x-gradient repeat bit for bit"""
    k = 8
    X = np.stack([np.concatenate(bc.random_pair(200, 600, dtype, seed=30 + b)[:1] * 2, 1) for b in range(3)])       # 6 columns
    Y = np.stack([np.concatenate([bc.random_pair(200, 600, dtype, seed=30 + b)[1]] * 2, 1) for b in range(3)])
    xr, yr = torch.tensor([200, 150, 0]).cuda(), torch.tensor([600, 5, 300]).cuda()
    runs = []
    for _ in range(2):
        xd, yd = torch.from_numpy(X).cuda().requires_grad_(True), torch.from_numpy(Y).cuda().requires_grad_(True)
        d2, idx = knn_points(xd, yd, k=k, x_rows=xr, y_rows=yr, method="grid")
        assert (idx[1, :150, 5:] == -1).all() and (idx[1, :150, :5] >= 0).all() and (idx[1, 150:] == -1).all() and (idx[2] == -1).all()
        g = torch.where(idx >= 0, torch.ones_like(d2), torch.full_like(d2, float("nan")))
        d2.backward(g)
        runs.append((d2.detach().cpu().numpy().tobytes(), idx.cpu().numpy().tobytes(), xd.grad.cpu().numpy().tobytes()))
        assert torch.isfinite(xd.grad).all() and torch.isfinite(yd.grad).all()
        assert (xd.grad[..., 3:] == 0).all() and (yd.grad[..., 3:] == 0).all()
        assert (xd.grad[1, 150:] == 0).all() and (xd.grad[2] == 0).all() and (xd.grad[1, :150, :3] != 0).any()
        assert (yd.grad[1, 5:] == 0).all() and (yd.grad[2] == 0).all() and (yd.grad[0, :, :3] != 0).any() and (yd.grad[1, :5, :3] != 0).all()
        assert not idx.requires_grad
        gx, gy = xd.grad.cpu().numpy(), yd.grad.cpu().numpy()
        i0 = idx[0].cpu().numpy()
        wl.knn_grad_check(X[0, :, :3], Y[0, :, :3], i0, np.ones(i0.shape, dtype), gx[0, :, :3], gy[0, :, :3], dtype, "cloud 0")
    assert runs[0] == runs[1]


# ------------------------------------------------------------------ 5. the Chamfer distance
def _cloud(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, 3), generator=g, dtype=torch.float64).to(dtype)


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_chamfer_against_float64_oracle_and_the_walk(reduction):
    N = 4
    x = torch.stack([_cloud(600, torch.float64, 60 + b) for b in range(N)])
    y = torch.stack([_cloud(450, torch.float64, 70 + b) for b in range(N)])
    xr, yr = [600, 200, 1, 600], [450, 450, 77, 2]
    xd = x.cuda().requires_grad_(True)
    yd = y.cuda().requires_grad_(True)
    val = chamfer_distance(xd, yd, x_rows=torch.tensor(xr), y_rows=torch.tensor(yr), reduction=reduction, method="grid")
    walk = chamfer_distance(x.cuda(), y.cuda(), x_rows=torch.tensor(xr), y_rows=torch.tensor(yr), reduction=reduction)
    assert torch.equal(val.detach(), walk)                  # the same nearest distances summed by the same code
    xo = [x[b, :xr[b]].clone().requires_grad_(True) for b in range(N)]
    yo = [y[b, :yr[b]].clone().requires_grad_(True) for b in range(N)]
    per = wl.chamfer_oracle(xo, yo)
    ref = per if reduction == "none" else (per.mean() if reduction == "mean" else per.sum())
    torch.testing.assert_close(val.cpu(), ref, rtol=1e-12, atol=1e-14)
    w = torch.randn(ref.shape, dtype=torch.float64)
    (val * w.cuda()).sum().backward()
    (ref * w).sum().backward()
    for b in range(N):
        torch.testing.assert_close(xd.grad[b, :xr[b]].cpu(), xo[b].grad, rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(yd.grad[b, :yr[b]].cpu(), yo[b].grad, rtol=1e-10, atol=1e-12)
        assert torch.all(xd.grad[b, xr[b]:] == 0) and torch.all(yd.grad[b, yr[b]:] == 0)


def test_chamfer_empty_clouds_and_forms():
    a, b = _cloud(50, torch.float32, 80), _cloud(40, torch.float32, 81)
    e = a[:0]
    v = chamfer_distance([a, e, e, a], [b, b, e, e], reduction="none", method="grid")
    assert v.shape == (4,) and v.device.type == "cpu"
    assert torch.isfinite(v[0]) and v[1] == float("inf") and v[2] == 0 and v[3] == float("inf")
    assert torch.equal(v, chamfer_distance([a, e, e, a], [b, b, e, e], reduction="none"))
    one = chamfer_distance(a, b, method="grid")
    assert one.shape == () and torch.equal(one, v[0])
    torch.testing.assert_close(chamfer_distance(a.double(), b.double(), method="grid"), wl.chamfer_oracle([a.double()], [b.double()])[0], rtol=1e-12, atol=0)
    assert chamfer_distance(a, e, method="grid") == float("inf") and chamfer_distance(e, e, method="grid") == 0


def test_chamfer_through_icp():
    from dicp_amd.ICP import ICP
    src, tgt = make_pairs(2, 500, 700, seed=4, dtype=torch.float64)
    s, t = src.cuda(), tgt[..., :3].contiguous().cuda()
    T0 = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1).cuda()
    w0 = torch.rand(2, 500, dtype=torch.float64).cuda() + 0.5

    def run(w):
        icp = ICP(icp_type="pt2pt", differentiable=True, max_iterations=3, tolerance=1e-12)
        icp.const_iter = True
        return icp.icp(s, t, T0, weight=w, trim_dist=5.0)["pc"]

    w1 = w0.clone().requires_grad_(True)
    chamfer_distance(run(w1), t, method="grid").backward()
    w2 = w0.clone().requires_grad_(True)
    pc = run(w2)
    pcs = [pc[b].detach().cpu().requires_grad_(True) for b in range(2)]
    wl.chamfer_oracle(pcs, [t[b].cpu() for b in range(2)]).mean().backward()
    pc.backward(torch.stack([p.grad for p in pcs]).cuda())
    assert w1.grad.abs().sum() > 0
    torch.testing.assert_close(w1.grad, w2.grad, rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------ 6. no host synchronisation, graph capture
def test_no_host_synchronisation():
    x, y = bc.random_pair(700, 5000, np.float32)
    xd, yd = torch.from_numpy(x).cuda().unsqueeze(0).requires_grad_(True), torch.from_numpy(y).cuda().unsqueeze(0).requires_grad_(True)
    xr, yr = torch.tensor([650], dtype=torch.int32).cuda(), torch.tensor([4000], dtype=torch.int32).cuda()
    knn_points(xd, yd, k=8, method="grid")                  # (the library is loaded)
    chamfer_distance(xd, yd, method="grid")
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        d2, idx = knn_points(xd, yd, k=8, x_rows=xr, y_rows=yr, method="grid")
        torch.where(idx >= 0, d2, torch.zeros_like(d2)).sum().backward()
        chamfer_distance(xd, yd, x_rows=xr, y_rows=yr, method="grid").backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert gh.same(_np((d2[0], idx[0])), gh.reference(x, y, 8, x_rows=650, y_rows=4000)) is None


def test_a_captured_call_replays_to_the_same_bits():
    x, y = bc.random_pair(700, 5000, np.float32)
    xs, ys = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    eager = knn_points(xs, ys, k=8, method="grid")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        knn_points(xs, ys, k=8, method="grid")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d2, idx = knn_points(xs, ys, k=8, method="grid")
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(idx, eager[1]) and d2.cpu().numpy().tobytes() == eager[0].cpu().numpy().tobytes()
    x2, y2 = bc.random_pair(700, 5000, np.float32, seed=1)  # other clouds through the same graph: nothing of the first is baked in
    xs.copy_(torch.from_numpy(x2))
    ys.copy_(torch.from_numpy(y2))
    graph.replay()
    torch.cuda.synchronize()
    assert gh.same(_np((d2, idx)), gh.reference(x2, y2, 8)) is None
