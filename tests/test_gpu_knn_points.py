"""knn_points and chamfer_distance on the MI355X against their definition (dicp_amd/knn.py): neighbours index for index and d2 bit for bit
against a numpy brute force that computes d2 with the same statements, the input forms and ragged rows, gradients against autograd, the
agreement with estimate_normals' own search, reproducibility, and the Chamfer distance alone and through a differentiable ICP call."""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.knn import chamfer_distance, knn_points
from dicp_amd.normals import estimate_normals
from dicp_amd.synthetic import make_pairs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from walk_layouts import chamfer_oracle as _chamfer_oracle, knn_oracle as _oracle  # noqa: E402  (the brute forces, shared with test_gpu_knn_walk.py)

pytestmark = pytest.mark.gpu


def _check(d2, idx, X, Y, k):
    d2o, io = _oracle(X, Y, k)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    bad = np.flatnonzero((idx != io).any(1))
    assert bad.size == 0, "%d queries differ, first %d: %s vs %s" % (bad.size, bad[0], idx[bad[0]], io[bad[0]])
    assert np.array_equal(d2.view(np.uint8), d2o.view(np.uint8))


def _cloud(n, dtype, seed, c=3, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((n, c), generator=g, dtype=torch.float64) * scale).to(dtype)


CASES = [(n, m, k, dt) for n, m in ((1, 1), (2, 17), (17, 2), (1000, 1000), (2049, 1000), (1000, 2049))
         for k, dt in zip((1, 2, 5, 8, 16, 17, 32), (torch.float32, torch.float64) * 4)]


@pytest.mark.parametrize("n,m,k,dtype", CASES)
def test_exact_against_brute_force(n, m, k, dtype):
    x, y = _cloud(n, dtype, n + 7 * k), _cloud(m, dtype, m + 11 * k + 1)
    d2, idx = knn_points(x.cuda(), y.cuda(), k=k)
    assert d2.shape == (n, k) and idx.shape == (n, k) and d2.dtype == dtype and idx.dtype == torch.int64
    _check(d2, idx, x.numpy(), y.numpy(), k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_hard_inputs(dtype):
    rng = np.random.default_rng(0)
    dt = np.float32 if dtype == torch.float32 else np.float64
    # integer grid: exact ties, duplicate rows
    Y = rng.integers(-3, 4, (600, 3)).astype(dt)
    Y[300:380] = Y[:80]
    X = (rng.integers(-4, 5, (500, 3)) * 0.5).astype(dt)
    # a wall perpendicular to x
    W = np.concatenate([np.zeros((500, 1)), rng.uniform(-1, 1, (500, 2))], 1).astype(dt)
    XW = np.concatenate([rng.uniform(-0.1, 0.1, (300, 1)), rng.uniform(-1, 1, (300, 2))], 1).astype(dt)
    # queries far outside the target's x range; NaN and huge rows
    F = rng.uniform(0, 1, (400, 3)).astype(dt)
    XF = rng.uniform(0, 1, (300, 3)).astype(dt)
    XF[:100, 0] += 100
    XF[100:200, 0] -= 100
    F[5, 0] = np.nan
    F[17, 1] = np.nan
    F[40:45] = np.finfo(dt).max / 2
    F[60, 2] = np.inf
    XF[200, 0] = np.nan
    XF[201, 2] = np.nan
    XF[202, 0] = np.inf
    XF[203] = np.finfo(dt).max / 2
    for Xn, Yn in ((X, Y), (XW, W), (XF, F), (X, Y[:5])):
        for k in (1, 4, 8, 32):
            d2, idx = knn_points(torch.from_numpy(Xn).cuda(), torch.from_numpy(Yn).cuda(), k=k)
            _check(d2, idx, Xn, Yn, k)


def test_large_batch_sampled():
    _, tgt = make_pairs(256, 16, 16384, seed=5)
    src, _ = make_pairs(256, 16384, 16, seed=6)
    x, y = src[..., :3].contiguous(), tgt[..., :3].contiguous()
    d2, idx = knn_points(x.cuda(), y.cuda(), k=8)
    for b in (0, 77, 170, 255):
        _check(d2[b], idx[b], x[b].numpy(), y[b].numpy(), 8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_ragged_rows_lists_single_and_cpu(dtype):
    N, n, m, k = 5, 300, 260, 6
    x = torch.stack([_cloud(n, dtype, 10 + b) for b in range(N)])
    y = torch.stack([_cloud(m, dtype, 20 + b) for b in range(N)])
    xr, yr = [300, 0, 17, 250, 1], [260, 100, 0, 3, 260]
    d2, idx = knn_points(x.cuda(), y.cuda(), k=k, x_rows=torch.tensor(xr), y_rows=torch.tensor(yr, dtype=torch.int32).cuda())
    for b in range(N):
        if xr[b]:
            d2o, io = _oracle(x[b, :xr[b]].numpy(), y[b, :yr[b]].numpy(), k)
            assert np.array_equal(idx[b, :xr[b]].cpu().numpy(), io)
            assert np.array_equal(d2[b, :xr[b]].cpu().numpy(), d2o)
        assert torch.all(idx[b, xr[b]:] == -1) and torch.all(d2[b, xr[b]:] == float("inf"))
    # lists: the same clouds cut to their rows; CPU in, CPU out
    xs, ys = [x[b, :xr[b]] for b in range(N)], [y[b, :yr[b]] for b in range(N)]
    dl, il = knn_points(xs, ys, k=k)
    assert len(dl) == N and all(t.device.type == "cpu" for t in dl + il)
    for b in range(N):
        assert dl[b].shape == (xr[b], k)
        assert torch.equal(il[b], idx[b, :xr[b]].cpu()) and torch.equal(dl[b], d2[b, :xr[b]].cpu())
    d1, i1 = knn_points(x[3], y[3], k=k)
    assert d1.device.type == "cpu" and torch.equal(i1, knn_points(x[3].cuda(), y[3].cuda(), k=k)[1].cpu())
    # an empty cloud on either side of a single pair
    d0, i0 = knn_points(x[0, :0], y[0], k=k)
    assert d0.shape == (0, k)
    d0, i0 = knn_points(x[0], y[0, :0], k=k)
    assert torch.all(i0 == -1) and torch.all(d0 == float("inf"))


def test_columns_three_and_six_zero_gradient_beyond_xyz():
    x6 = _cloud(400, torch.float64, 1, c=6).cuda().requires_grad_(True)
    y6 = _cloud(300, torch.float64, 2, c=6).cuda().requires_grad_(True)
    d2, idx = knn_points(x6, y6, k=4)
    d23, idx3 = knn_points(x6[:, :3].detach(), y6[:, :3].detach(), k=4)
    assert torch.equal(idx, idx3) and torch.equal(d2.detach(), d23)
    g = torch.randn_like(d2)
    (d2 * g).sum().backward()
    assert torch.all(x6.grad[:, 3:] == 0) and torch.all(y6.grad[:, 3:] == 0)
    assert x6.grad[:, :3].abs().sum() > 0 and y6.grad[:, :3].abs().sum() > 0


@pytest.mark.parametrize("k", [3, 8, 16, 32])
def test_self_search_matches_estimate_normals(k):
    p = _cloud(1500, torch.float32, 9).cuda()
    _, idx = knn_points(p, p, k=k)
    _, nbr = estimate_normals(p, k=k, return_neighbors=True)
    assert torch.equal(idx, nbr)


def test_gradcheck_float64():
    x = _cloud(40, torch.float64, 3).cuda().requires_grad_(True)
    y = _cloud(30, torch.float64, 4).cuda().requires_grad_(True)
    for k in (1, 5):
        assert torch.autograd.gradcheck(lambda a, b: knn_points(a, b, k=k)[0], (x, y), eps=1e-7, atol=1e-6)


def _autograd_oracle(x, y, idx, g):
    """float64 autograd of sum g * |x_i - y_idx|^2 over the idx >= 0 entries"""
    x64 = x.detach().double().cpu().requires_grad_(True)
    y64 = y.detach().double().cpu().requires_grad_(True)
    idx = idx.cpu()
    ok = idx >= 0
    yy = y64[..., :3].gather(-2, idx.clamp(min=0).reshape(*idx.shape[:-2], -1, 1).expand(*idx.shape[:-2], -1, 3)).reshape(*idx.shape, 3)
    d = x64[..., None, :3] - yy
    val = (d * d).sum(-1)
    (torch.where(ok, val, torch.zeros_like(val)) * g.double().cpu()).sum().backward()
    return x64.grad, y64.grad


def test_float32_gradients_against_float64_autograd():
    N = 3
    x = torch.stack([_cloud(700, torch.float32, 30 + b) for b in range(N)]).cuda().requires_grad_(True)
    y = torch.stack([_cloud(500, torch.float32, 40 + b) for b in range(N)]).cuda().requires_grad_(True)
    xr, yr = torch.tensor([700, 300, 0]), torch.tensor([500, 5, 200])
    d2, idx = knn_points(x, y, k=7, x_rows=xr, y_rows=yr)
    g = torch.randn_like(d2)
    (torch.where(idx >= 0, d2, torch.zeros_like(d2)) * g).sum().backward()
    gx, gy = _autograd_oracle(x, y, idx, torch.where(idx >= 0, g, torch.zeros_like(g)))
    torch.testing.assert_close(x.grad.double().cpu(), gx, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(y.grad.double().cpu(), gy, rtol=1e-5, atol=1e-5)
    assert torch.all(x.grad[1, 300:] == 0) and torch.all(y.grad[1, 5:] == 0)


def test_forward_and_x_gradient_bit_reproducible():
    x = _cloud(5000, torch.float32, 50).cuda()
    y = _cloud(4000, torch.float32, 51).cuda()
    g = torch.randn((5000, 16), device="cuda")
    outs = []
    for _ in range(2):
        xi = x.clone().requires_grad_(True)
        d2, idx = knn_points(xi, y, k=16)
        (d2 * g).sum().backward()
        outs.append((d2.detach(), idx, xi.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- Chamfer distance

@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_chamfer_against_float64_oracle(reduction):
    N = 4
    x = torch.stack([_cloud(600, torch.float64, 60 + b) for b in range(N)])
    y = torch.stack([_cloud(450, torch.float64, 70 + b) for b in range(N)])
    xr, yr = [600, 200, 1, 600], [450, 450, 77, 2]
    xd = x.cuda().requires_grad_(True)
    yd = y.cuda().requires_grad_(True)
    val = chamfer_distance(xd, yd, x_rows=torch.tensor(xr), y_rows=torch.tensor(yr), reduction=reduction)
    xo = [x[b, :xr[b]].clone().requires_grad_(True) for b in range(N)]
    yo = [y[b, :yr[b]].clone().requires_grad_(True) for b in range(N)]
    per = _chamfer_oracle(xo, yo)
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
    v = chamfer_distance([a, e, e, a], [b, b, e, e], reduction="none")
    assert v.shape == (4,) and v.device.type == "cpu"
    assert torch.isfinite(v[0]) and v[1] == float("inf") and v[2] == 0 and v[3] == float("inf")
    one = chamfer_distance(a, b)
    assert one.shape == () and torch.equal(one, v[0])
    torch.testing.assert_close(chamfer_distance(a.double(), b.double()), _chamfer_oracle([a.double()], [b.double()])[0], rtol=1e-12, atol=0)
    assert chamfer_distance(a, e) == float("inf") and chamfer_distance(e, e) == 0


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
    chamfer_distance(run(w1), t).backward()

    w2 = w0.clone().requires_grad_(True)
    pc = run(w2)
    pcs = [pc[b].detach().cpu().requires_grad_(True) for b in range(2)]
    ref = _chamfer_oracle(pcs, [t[b].cpu() for b in range(2)]).mean()
    ref.backward()
    pc.backward(torch.stack([p.grad for p in pcs]).cuda())
    torch.testing.assert_close(w1.grad, w2.grad, rtol=1e-9, atol=1e-9)
