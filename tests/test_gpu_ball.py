"""ball_query on the MI355X against its definition (dicp_amd/ball.py): index for index, d2 bit for bit and counts exactly against the numpy
brute force tests/ball_ref.py -- random cubes, the integer lattice on the bound, degenerate layouts (one cell, lines, a wall, clusters that
need the enlarged edge, underflow, far queries), non-finite and ragged rows and every input form; against masked knn_points; the gradients
against an autograd graph built from the returned indices; reproducibility; no host synchronisation; and the voxel -> FPS -> ball chain."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.ball import ball_query
from dicp_amd.fps import sample_farthest_points
from dicp_amd.knn import knn_points
from dicp_amd.voxel import voxel_downsample

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ball_clouds as bc  # noqa: E402
from ball_ref import ball_ref, r2_of, same  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
KMAX = max(bc.KS)


def _np(outs):
    return tuple(o.detach().cpu().numpy() for o in outs)


def _hold(x, y, radius, ks=bc.KS, ref=None):
    """one pair of clouds on the device at every k against the reference at the largest k (its leading columns are the smaller k's)"""
    ref = ref if ref is not None else ball_ref(x, y, radius, max(ks))
    xd, yd = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(y)).cuda()
    for k in ks:
        d2, idx, counts = ball_query(xd, yd, radius, k=k, return_counts=True)
        n = x.shape[0]
        assert d2.shape == (n, k) and idx.shape == (n, k) and counts.shape == (n,)
        assert d2.dtype == xd.dtype and idx.dtype == torch.int64 and counts.dtype == torch.int32
        bad = same(_np((d2, idx, counts)), (ref[0][:, :k], ref[1][:, :k], ref[2]))
        assert bad is None, "k=%d: %s" % (k, bad)
    return ref


@functools.lru_cache(maxsize=None)
def _random_ref(n, m, dtype, r):
    x, y = bc.random_pair(n, m, dtype)
    ref = ball_ref(x, y, r, KMAX)
    for a in (x, y) + ref:
        a.setflags(write=False)
    return x, y, ref


# ------------------------------------------------------------------ 1. random cubes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", bc.RANDOM_SHAPES)
def test_random_cubes(n, m, dtype):
    for r in bc.RANDOM_RADII:
        x, y, ref = _random_ref(n, m, dtype, r)
        _hold(x, y, r, ref=ref)
        if r == 2.0:
            assert (ref[2] == m).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_cubes_cover_every_kind_of_query(dtype):
    c = np.concatenate([_random_ref(n, m, dtype, r)[2][2] for n, m in bc.RANDOM_SHAPES for r in bc.RANDOM_RADII])
    for k in bc.KS:
        assert (c == 0).any() and ((c > 0) & (c <= k)).any() and (c > k).any()


def test_a_cloud_of_many_sort_chunks():
    """20000 rows: 32768 sorted slots, 16 LDS chunks and every stride of the sort between them"""
    x, y = bc.random_pair(300, 20000, np.float32)
    ref = _hold(x, y, 0.05, ks=(8,))
    assert (ref[2] > 8).any() and (ref[2] < 8).any()


# ------------------------------------------------------------------ 2. boundaries
@pytest.mark.parametrize("dtype", DTYPES)
def test_lattice_on_the_bound(dtype):
    centre, want = 171, {1.0: 7, 1.5: 19, 2.0: 33}
    for name, x, y, r in bc.lattice_cases(dtype):
        ref = _hold(x, y, r)
        if name.startswith("lattice r=") and r in want:
            assert ref[2][centre] == want[r], name
        if name == "lattice r=%r" % float(np.sqrt(dtype(2))):
            assert ref[2][centre] == (7 if dtype == np.float32 else 19)              # r2 = 1.9999999 / 2.0000000000000004: the dtype decides


# ------------------------------------------------------------------ 3. degenerate layouts
@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_layouts(dtype):
    names = set()
    for name, x, y, r in bc.degenerate_cases(dtype):
        ref = _hold(x, y, r)
        names.add(name)
        if name == "300 copies":
            assert ref[2].tolist() == [300, 300, 0]
        if name == "underflow":
            assert ref[2].tolist() == [2]
        if name == "far queries":
            assert ref[2][:4].tolist() == [0, 0, 0, 0] and ref[2][5] > 0
        if name == "two clusters":
            assert (ref[2] > 1).any()
    assert {"300 copies", "line along z", "line along x", "wall", "two clusters", "far queries"} <= names
    assert ("underflow" in names) == (dtype == np.float32)


# ------------------------------------------------------------------ 4. non-finite and ragged rows, input forms
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_rows(dtype):
    x, y = bc.nonfinite_pair(dtype)
    ref = _hold(x, y, 0.15)
    assert ref[2][[0, 7, 150]].tolist() == [0, 0, 0] and (ref[1][[0, 7, 150]] == -1).all()
    assert not np.isin(ref[1], [5, 17, 400, 899]).any()
    big = np.array([[3.0e38, 0, 0], [-3.0e38, 0, 0], [0, 0, 0], [0, 1, 0]], dtype=dtype)           # float32: the extent overflows -> one cell
    assert _hold(big[2:], big, 1.5, ks=(8,))[2].tolist() == [2, 2]
    big = np.array([[1.0e19, 0, 0], [-1.0e19, 0, 0], [0, 0, 0], [0, 1, 0]], dtype=dtype)           # float32: r2 = +inf, only finite d2 count
    assert _hold(big, big, 1.0e30, ks=(8,))[2].tolist() == ([3, 3, 4, 4] if dtype == np.float32 else [4, 4, 4, 4])


@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_batches_and_input_forms(dtype):
    tdt = TORCH[dtype]
    r, k = 0.15, 8
    sizes = ((300, 900), (120, 0), (0, 500), (257, 40), (1, 1))
    clouds = [bc.random_pair(max(n, 1), max(m, 1), dtype, seed=20 + i) for i, (n, m) in enumerate(sizes)]
    clouds = [(x[:n], y[:m]) for (x, y), (n, m) in zip(clouds, sizes)]
    clouds[0] = bc.nonfinite_pair(dtype)
    refs = [ball_ref(x, y, r, k) for x, y in clouds]
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
            d2, idx, counts = ball_query(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), r, k=k, x_rows=xr.to(rows_dev), y_rows=yr.to(rows_dev),
                                         return_counts=True)
            assert d2.shape == (N, n_max, k) and counts.shape == (N, n_max)
            d2, idx, counts = _np((d2, idx, counts))
            for b, (n, m) in enumerate(sizes):
                bad = same((d2[b, :n], idx[b, :n], counts[b, :n]), refs[b])
                assert bad is None, "%s cloud %d: %s" % (fill, b, bad)
                assert np.isinf(d2[b, n:]).all() and (idx[b, n:] == -1).all() and (counts[b, n:] == 0).all()
    # lists
    ld2, lidx, lcnt = ball_query([torch.from_numpy(x).cuda() for x, _ in clouds], [torch.from_numpy(y).cuda() for _, y in clouds], r, k=k, return_counts=True)
    for b, (n, m) in enumerate(sizes):
        assert ld2[b].shape == (n, k) and lcnt[b].shape == (n,)
        assert same(_np((ld2[b], lidx[b], lcnt[b])), refs[b]) is None
    # single clouds on the device and from the CPU, 6 columns, a non-contiguous view, m = 0 and n = 0
    x, y = clouds[0]
    for dev in ("cuda", "cpu"):
        outs = ball_query(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), r, k=k, return_counts=True)
        assert all(o.device.type == dev for o in outs) and outs[0].dtype == tdt
        assert same(_np(outs), refs[0]) is None
        assert len(ball_query(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), r, k=k)) == 2
    x6 = torch.from_numpy(np.concatenate([x, x + 5], 1)).cuda()
    y6 = torch.from_numpy(np.concatenate([y, y - 5], 1)).cuda()
    assert same(_np(ball_query(x6, y6, r, k=k, return_counts=True)), refs[0]) is None
    wide = torch.from_numpy(np.concatenate([y, y, y], 1)).cuda()[:, 3:7]
    assert not wide.is_contiguous()
    assert same(_np(ball_query(torch.from_numpy(x).cuda(), wide, r, k=k, return_counts=True)), refs[0]) is None
    assert same(_np(ball_query(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.tensor(r, dtype=torch.float64).cuda(), k=k, return_counts=True)),
                refs[0]) is None                             # a radius that lives on the device
    e = ball_query(torch.from_numpy(x).cuda(), torch.zeros((0, 3), dtype=tdt).cuda(), r, k=k, return_counts=True)
    assert e[0].shape == (300, k) and torch.isinf(e[0]).all() and (e[1] == -1).all() and (e[2] == 0).all()
    e = ball_query(torch.zeros((0, 3), dtype=tdt).cuda(), torch.from_numpy(y).cuda(), r, k=k, return_counts=True)
    assert e[0].shape == (0, k) and e[1].shape == (0, k) and e[2].shape == (0,)


# ------------------------------------------------------------------ 5. against knn_points
@pytest.mark.parametrize("dtype", DTYPES)
def test_equals_masked_knn_points(dtype):
    wall = bc.wall_pair(400, 3000, dtype)
    for (x, y), r in ((bc.random_pair(700, 5000, dtype), 0.05), (bc.random_pair(700, 5000, dtype), 0.1), (bc.random_pair(3000, 300, dtype), 0.2), (wall, 0.05)):
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        r2 = torch.tensor(r2_of(r, dtype)).cuda()
        for k in bc.KS:
            kd2, kidx = knn_points(xd, yd, k=k)
            out = kd2 > r2
            kd2 = torch.where(out, torch.full_like(kd2, float("inf")), kd2)
            kidx = torch.where(out, torch.full_like(kidx, -1), kidx)
            d2, idx = ball_query(xd, yd, r, k=k)
            assert torch.equal(idx, kidx) and d2.cpu().numpy().tobytes() == kd2.cpu().numpy().tobytes()


# ------------------------------------------------------------------ 6. gradients
def _grad_case(x, y, radius, k, dtype, seed, nan_at_empty=False):
    """x.grad / y.grad of sum(g * d2) against the autograd graph that forms d2 from the returned idx in float64: a component passes within
    (terms + 1) u_T sum|t| of the float64 sum of its terms t = 2 g (x - y) -- any summation order of the atomics, safety factor 1 -- and is
    checked only where that bound is under a quarter of its smallest |t| (one lost or doubled term fails).  Returns the share left out."""
    tdt = TORCH[dtype]
    u = float(np.finfo(dtype).eps) / 2
    gen = torch.Generator().manual_seed(seed)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    yd = torch.from_numpy(y).cuda().requires_grad_(True)
    d2, idx = ball_query(xd, yd, radius, k=k)
    g = ((torch.rand(d2.shape, generator=gen, dtype=torch.float64) * 1.5 + 0.5) * (torch.randint(0, 2, d2.shape, generator=gen) * 2 - 1)).to(tdt).cuda()
    live = idx >= 0
    assert live.any() and ((~live).any() or not nan_at_empty)
    cot = torch.where(live, g, torch.full_like(g, float("nan"))) if nan_at_empty else g
    d2.backward(cot)
    gx, gy = xd.grad.double(), yd.grad.double()
    assert torch.isfinite(gx).all() and torch.isfinite(gy).all()
    # the terms, in float64
    xs, ys = xd.detach().double(), yd.detach().double()
    safe = idx.clamp(min=0)
    t = 2.0 * g.double()[..., None] * (xs[:, None, :3] - ys[safe][..., :3])          # (n, k, 3)
    t = torch.where(live[..., None], t, torch.zeros_like(t))
    ref_x, abs_x, cnt_x = t.sum(1), t.abs().sum(1), live.sum(1)[:, None].expand(-1, 3)
    big = torch.full_like(t, float("inf"))
    min_x = torch.where(live[..., None], t.abs(), big).amin(1)
    m = y.shape[0]
    flat = safe.reshape(-1)
    ref_y = torch.zeros((m, 3), dtype=torch.float64, device="cuda").index_add_(0, flat, -t.reshape(-1, 3))
    abs_y = torch.zeros((m, 3), dtype=torch.float64, device="cuda").index_add_(0, flat, t.abs().reshape(-1, 3))
    cnt_y = torch.zeros(m, dtype=torch.int64, device="cuda").index_add_(0, flat, live.reshape(-1).long())[:, None].expand(-1, 3)
    min_y = torch.full((m, 3), float("inf"), dtype=torch.float64, device="cuda").scatter_reduce_(
        0, flat[:, None].expand(-1, 3), torch.where(live[..., None], t.abs(), big).reshape(-1, 3), "amin")
    # the same graph through autograd, as a check of the bookkeeping above
    xa, ya = xs.clone().requires_grad_(True), ys.clone().requires_grad_(True)
    da = ((ya[safe][..., :3] - xa[:, None, :3]) ** 2).sum(-1)
    (torch.where(live, da, torch.zeros_like(da)) * g.double()).sum().backward()
    assert torch.allclose(xa.grad[:, :3], ref_x, rtol=1e-12, atol=1e-14) and torch.allclose(ya.grad[:, :3], ref_y, rtol=1e-12, atol=1e-14)
    skipped = total = 0
    for got, ref, ab, cnt, mn in ((gx[:, :3], ref_x, abs_x, cnt_x, min_x), (gy[:, :3], ref_y, abs_y, cnt_y, min_y)):
        bound = (cnt + 1).double() * u * ab
        none = cnt == 0
        assert (got[none] == 0).all()                       # rows without a term: exactly zero
        checked = ~none & (bound < 0.25 * mn)
        assert ((got - ref).abs() <= bound)[~none].all(), float(((got - ref).abs() - bound)[~none].max())    # (the bound holds everywhere;
        skipped += int((~none & ~checked).sum())            # where it is not under a quarter of the smallest term it shows less)
        total += int((~none).sum())
    if x.shape[1] > 3:
        assert (gx[:, 3:] == 0).all() and (gy[:, 3:] == 0).all()
    return skipped / max(total, 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients(dtype):
    x, y = bc.random_pair(700, 5000, dtype)
    assert _grad_case(x, y, 0.1, 8, dtype, 1) <= 0.05
    x6, y6 = np.concatenate([x, x], 1), np.concatenate([y, y], 1)
    assert _grad_case(x6, y6, 0.05, 8, dtype, 2, nan_at_empty=True) <= 0.05                 # empty slots, NaN cotangents there, extra columns
    rng = np.random.default_rng(3)
    yk = np.concatenate([np.array([[0.5, 0.5, 0.5]]), rng.random((400, 3)) * 0.2 + 2.0]).astype(dtype)
    xk = (0.5 + (rng.random((300, 3)) - 0.5) * 0.1).astype(dtype)                           # 300 queries around row 0 of y: in-degree 300
    assert _grad_case(xk, yk, 0.2, 8, dtype, 4) <= 0.05


@pytest.mark.parametrize("dtype", DTYPES)
def test_pad_rows_get_zero_gradient_and_runs_repeat(dtype):
    X = np.stack([bc.random_pair(200, 600, dtype, seed=30 + b)[0] for b in range(3)])
    Y = np.stack([bc.random_pair(200, 600, dtype, seed=30 + b)[1] for b in range(3)])
    xr, yr = torch.tensor([200, 150, 0]).cuda(), torch.tensor([600, 0, 300]).cuda()
    runs = []
    for _ in range(2):
        xd, yd = torch.from_numpy(X).cuda().requires_grad_(True), torch.from_numpy(Y).cuda().requires_grad_(True)
        d2, idx, counts = ball_query(xd, yd, 0.15, k=8, x_rows=xr, y_rows=yr, return_counts=True)
        g = torch.where(idx >= 0, torch.ones_like(d2), torch.full_like(d2, float("nan")))
        g[1, 150:] = float("inf")                           # whatever arrives at pad rows and empty slots
        d2.backward(g)
        runs.append((d2.detach().cpu().numpy().tobytes(), idx.cpu().numpy().tobytes(), counts.cpu().numpy().tobytes(), xd.grad.cpu().numpy().tobytes()))
        assert torch.isfinite(xd.grad).all() and torch.isfinite(yd.grad).all()
        assert (xd.grad[1, 150:] == 0).all() and (xd.grad[2] == 0).all() and (xd.grad[1] == 0).all()
        assert (yd.grad[1] == 0).all() and (yd.grad[2] == 0).all() and (yd.grad[0] != 0).any()
        assert not counts.requires_grad and not idx.requires_grad
    assert runs[0] == runs[1]                               # the forward and the x-gradient, bit for bit


# ------------------------------------------------------------------ 7. no host synchronisation, the chain
def test_no_host_synchronisation():
    x, y = bc.random_pair(700, 5000, np.float32)
    xd, yd = torch.from_numpy(x).cuda().unsqueeze(0).requires_grad_(True), torch.from_numpy(y).cuda().unsqueeze(0)
    xr, yr = torch.tensor([650], dtype=torch.int32).cuda(), torch.tensor([4000], dtype=torch.int32).cuda()
    ball_query(xd, yd, 0.1, k=8)                            # (the library is loaded)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        d2, idx, counts = ball_query(xd, yd, 0.1, k=8, x_rows=xr, y_rows=yr, return_counts=True)
        torch.where(idx >= 0, d2, torch.zeros_like(d2)).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    ref = ball_ref(x, y, 0.1, 8, x_rows=650, y_rows=4000)
    assert same(_np((d2[0], idx[0], counts[0])), ref) is None


def test_voxel_fps_ball_chain():
    rng = np.random.default_rng(11)
    scan = torch.from_numpy(rng.random((2, 6000, 3)).astype(np.float32) * np.float32(4.0)).cuda().requires_grad_(True)
    rows = torch.tensor([6000, 4500], dtype=torch.int32).cuda()
    cloud, crow = voxel_downsample(scan, 0.2, rows=rows)
    centres, _, erow = sample_farthest_points(cloud, 64, rows=crow, return_rows=True)
    d2, idx, counts = ball_query(centres, cloud, 0.5, 16, x_rows=erow, y_rows=crow, return_counts=True)
    assert d2.shape == (2, 64, 16)
    cn, yn = centres.detach().cpu().numpy(), cloud.detach().cpu().numpy()
    for b in range(2):
        ref = ball_ref(cn[b], yn[b], 0.5, 16, x_rows=int(erow[b]), y_rows=int(crow[b]))
        assert same(_np((d2[b], idx[b], counts[b])), ref) is None
        assert (ref[2] >= 1).all()                          # every centre is a row of the cloud
    torch.where(idx >= 0, d2, torch.zeros_like(d2)).sum().backward()
    g = scan.grad
    assert torch.isfinite(g).all() and (g[0] != 0).any() and (g[1, :4500] != 0).any() and (g[1, 4500:] == 0).all()
