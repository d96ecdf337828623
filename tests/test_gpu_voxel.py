"""voxel_downsample on the MI355X against its definition (dicp_amd/voxel.py): rows_out, voxel order, counts and inverse exactly as a numpy
oracle computes them (np.floor in the points' dtype, np.unique(axis=0), a float64 np.add.at mean), centroids to the rounding the definition
allows; ignored rows, scale, plumbing, bit-reproducibility, gradients, and the voxel_downsample -> estimate_normals -> pt2pl ICP chain."""
import numpy as np
import pytest
import torch

from dicp_amd.ICP import ICP
from dicp_amd.normals import estimate_normals
from dicp_amd.synthetic import make_pairs, make_scene_pairs
from dicp_amd.voxel import voxel_downsample

pytestmark = pytest.mark.gpu


def _oracle(P, size, origin, min_points):
    """P (m, c) numpy in its own dtype (the cloud's own rows) -> (centroids float64 (V, c), counts (V,), inverse (m,), max |member| per voxel (V, c))"""
    dt = P.dtype.type
    s = np.broadcast_to(np.asarray(size, dtype=np.float64), (3,)).astype(P.dtype)
    o = np.zeros(3, dtype=P.dtype) if origin is None else np.asarray(origin, dtype=np.float64).astype(P.dtype)
    inverse = np.full(P.shape[0], -1, dtype=np.int64)
    idx = np.flatnonzero(np.isfinite(P[:, :3]).all(1))
    if idx.size == 0:
        return np.zeros((0, P.shape[1])), np.zeros(0, dtype=np.int64), inverse, np.zeros((0, P.shape[1]))
    V = np.floor((P[idx, :3] - o) / s).astype(np.int64)
    assert V.dtype == np.int64 and (P[idx, :3] - o).dtype == dt
    uniq, inv, cnt = np.unique(V, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    sums = np.zeros((uniq.shape[0], P.shape[1]), dtype=np.float64)
    np.add.at(sums, inv, P[idx].astype(np.float64))
    big = np.zeros_like(sums)
    np.maximum.at(big, inv, np.abs(P[idx].astype(np.float64)))
    keep = cnt >= min_points
    new = np.cumsum(keep) - 1
    inverse[idx] = np.where(keep[inv], new[inv], -1)
    return (sums / cnt[:, None])[keep], cnt[keep], inverse, big[keep]


def _check_cloud(cent, counts, inverse, P, size, origin=None, min_points=1):
    """one cloud's outputs (numpy, already cut to its voxels / rows) against the oracle"""
    ref, rc, rinv, big = _oracle(P, size, origin, min_points)
    assert cent.shape[0] == ref.shape[0], (cent.shape, ref.shape)
    assert np.array_equal(counts, rc)
    assert np.array_equal(inverse, rinv)
    if P.dtype == np.float32:
        r32 = ref.astype(np.float32)
        assert np.all(np.abs(cent.astype(np.float64) - r32.astype(np.float64)) <= np.spacing(np.abs(r32)).astype(np.float64))
    else:
        tol = rc[:, None] * 2.0 ** -52 * big
        assert np.all(np.abs(cent - ref) <= tol)


def _check_batch(pts, size, rows=None, origin=None, min_points=1, clouds=None):
    """pts (N, m, c) torch CPU; the GPU call on the batch, every cloud (or those listed) against the oracle"""
    N, m, c = pts.shape
    rows_t = None if rows is None else torch.tensor(rows, dtype=torch.int32).cuda()
    cent, ro, cnt, inv = voxel_downsample(pts.cuda(), size, rows=rows_t, origin=origin, min_points=min_points, return_counts=True, return_inverse=True)
    assert cent.dtype == pts.dtype and ro.dtype == torch.int32 and cnt.dtype == torch.int32 and inv.dtype == torch.int64
    cent, ro, cnt, inv = cent.cpu().numpy(), ro.cpu().numpy(), cnt.cpu().numpy(), inv.cpu().numpy()
    assert cent.shape == (N, ro.max(), c) and cnt.shape == (N, ro.max()) and inv.shape == (N, m)
    org = None if origin is None else np.asarray(origin, dtype=np.float64)
    for b in (range(N) if clouds is None else clouds):
        mb = m if rows is None else rows[b]
        o_b = None if org is None else (org if org.ndim == 1 else org[b])
        r = int(ro[b])
        _check_cloud(cent[b, :r], cnt[b, :r], inv[b, :mb], pts[b, :mb].numpy(), size, o_b, min_points)
        assert np.all(cent[b, r:] == 0) and np.all(cnt[b, r:] == 0) and np.all(inv[b, mb:] == -1)
    return ro


def _uniform(N, m, c, dtype, seed, scale=4.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand((N, m, c), generator=g, dtype=torch.float64) - 0.5) * scale + shift).to(dtype)


DTYPES = [torch.float32, torch.float64]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [3, 4, 6])
def test_exact_scalar_size(dtype, c):
    _check_batch(_uniform(3, 20000, c, dtype, seed=c), 0.25)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_per_axis_size_and_cloud_origins(dtype):
    pts = _uniform(4, 15000, 4, dtype, seed=7, scale=6.0)
    origin = np.array([[0.1, -0.3, 0.05], [0.0, 0.0, 0.0], [-2.5, 1.0, 3.3], [0.01, 0.02, 0.03]])
    _check_batch(pts, [0.3, 0.17, 0.41], origin=torch.tensor(origin))
    _check_batch(pts, torch.tensor([0.5, 0.5, 0.05]), origin=[1.0, 2.0, -1.0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("min_points", [2, 5, 40])
def test_exact_min_points(dtype, min_points):
    ro = _check_batch(_uniform(3, 12000, 3, dtype, seed=min_points), 0.35, min_points=min_points)
    if min_points == 40:
        assert ro.max() < _check_batch(_uniform(3, 12000, 3, dtype, seed=min_points), 0.35).max()


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_points_in_one_voxel(dtype):
    pts = _uniform(2, 50000, 4, dtype, seed=3, scale=0.9, shift=0.5)     # (0.05, 0.95) in every column
    ro = _check_batch(pts, 1.0)
    assert list(ro) == [1, 1]
    ro = _check_batch(pts[:, :300], 1.0)                                    # a voxel just past the per-lane size
    assert list(ro) == [1, 1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_point_its_own_voxel(dtype):
    g = torch.Generator().manual_seed(5)
    cells = torch.randperm(60 ** 3, generator=g)[:30000]
    pts = torch.stack((cells // 3600, (cells // 60) % 60, cells % 60), 1).to(torch.float64) * 0.25 + 0.1 - 7.5
    pts = torch.cat((pts, torch.rand((30000, 2), generator=g, dtype=torch.float64)), 1).unsqueeze(0).to(dtype)
    ro = _check_batch(pts, 0.25)
    assert ro[0] == 30000


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicates(dtype):
    g = torch.Generator().manual_seed(9)
    pts = (torch.randint(-6, 6, (2, 8000, 3), generator=g).to(torch.float64) * 0.25).to(dtype)      # on the faces, ~14 copies each
    pts = torch.cat((pts, torch.rand((2, 8000, 2), generator=g, dtype=torch.float64).to(dtype)), -1)
    _check_batch(pts, 0.25)
    _check_batch(pts, 0.5, min_points=20)


@pytest.mark.parametrize("dtype", DTYPES)
def test_far_from_origin(dtype):
    pts = _uniform(2, 20000, 3, dtype, seed=13, scale=30.0, shift=0.0)
    pts = (pts.to(torch.float64) + torch.tensor([2500.0, -1800.0, 300.0], dtype=torch.float64)).to(dtype)
    _check_batch(pts, 0.1)
    _check_batch(pts, 0.07, origin=torch.tensor([[2500.0, -1800.0, 300.0], [2400.0, -1700.0, 250.0]]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ignored_rows(dtype):
    pts = _uniform(4, 5000, 4, dtype, seed=17)
    rows = [5000, 3100, 0, 1]
    pts[1, 3100:] = float("nan")
    pts[3, 1:] = 1e30
    pts[0, 10, 0] = float("nan")
    pts[0, 11, 1] = float("inf")
    pts[0, 12, 2] = -float("inf")
    pts[0, 13, 3] = float("nan")                             # a non-xyz column: the row takes part (its centroid is NaN)
    pts[1, 100:200, 2] = float("nan")
    ro = _check_batch(pts[:, :, :3].contiguous(), 0.5, rows=rows)
    assert ro[2] == 0 and ro[3] == 1
    cent, ro, inv = voxel_downsample(pts.cuda(), 0.5, rows=torch.tensor(rows), return_inverse=True)
    inv = inv.cpu()
    assert torch.all(inv[0, 10:13] == -1) and inv[0, 13] >= 0 and torch.all(inv[1, 100:200] == -1) and torch.all(inv[2] == -1)
    cent = cent.cpu()
    assert torch.isnan(cent[0, int(inv[0, 13]), 3]).item() and int(torch.isnan(cent[0]).any(1).sum()) == 1


def test_no_valid_rows_anywhere():
    pts = torch.full((2, 100, 3), float("nan"))
    cent, ro, cnt, inv = voxel_downsample(pts.cuda(), 0.1, return_counts=True, return_inverse=True)
    assert cent.shape == (2, 0, 3) and cnt.shape == (2, 0) and torch.all(ro.cpu() == 0) and torch.all(inv.cpu() == -1)


def test_range_errors_name_the_cloud():
    pts = _uniform(3, 1000, 3, torch.float64, seed=1)
    bad = pts.clone()
    bad[1, 5, 0] = 2.0 ** 62
    with pytest.raises(ValueError, match="cloud 1"):
        voxel_downsample(bad.cuda(), 1.0)
    wide = pts.clone()
    wide[2, 0] = torch.tensor([-(2.0 ** 21), -(2.0 ** 20), -(2.0 ** 20)], dtype=torch.float64)
    wide[2, 1] = torch.tensor([2.0 ** 21 - 1, 2.0 ** 20 - 1, 2.0 ** 20 - 1], dtype=torch.float64)      # spans of 22 + 21 + 21 = 64 bits: fine
    ro = _check_batch(wide[2:3].contiguous(), 1.0)                                                    # (the oracle's voxels, order and means)
    assert ro[0] >= 3
    wide[2, 1, 1] = 2.0 ** 20                                                                          # 22 + 22 + 21 = 65
    with pytest.raises(ValueError, match="cloud 2"):
        voxel_downsample(wide.cuda(), 1.0)


@pytest.mark.parametrize("gen", ["scene", "pairs"])
def test_scale_batch(gen):
    N, m = 256, 131072
    _, tgt = (make_scene_pairs if gen == "scene" else make_pairs)(N, 16, m, seed=3, dtype=torch.float32)
    pts = tgt[..., :3].contiguous()
    size = 0.1 if gen == "scene" else 0.8
    cent, ro, cnt, inv = voxel_downsample(pts.cuda(), size, return_counts=True, return_inverse=True)
    cent, ro, cnt, inv = cent.cpu().numpy(), ro.cpu().numpy(), cnt.cpu().numpy(), inv.cpu().numpy()
    assert ro.min() > 0 and ro.max() < m
    for b in np.random.default_rng(4).choice(N, 6, replace=False):
        r = int(ro[b])
        _check_cloud(cent[b, :r], cnt[b, :r], inv[b], pts[b].numpy(), size)


def test_scale_single_map():
    m = 4194304
    g = torch.Generator().manual_seed(21)
    xy = (torch.rand((m, 2), generator=g, dtype=torch.float64) - 0.5) * 200.0
    z = 0.5 * torch.sin(0.1 * xy[:, :1]) + 0.05 * torch.randn((m, 1), generator=g, dtype=torch.float64)
    pts = torch.cat((xy, z), 1).to(torch.float32)
    cent, ro, cnt, inv = voxel_downsample(pts.cuda(), 0.2, return_counts=True, return_inverse=True)
    assert cent.shape[0] == int(ro) and inv.shape == (m,)
    _check_cloud(cent.cpu().numpy(), cnt.cpu().numpy(), inv.cpu().numpy(), pts.numpy(), 0.2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_forms_agree_and_cpu_in_cpu_out(dtype):
    lens = [3000, 17, 1, 5000]
    g = torch.Generator().manual_seed(31)
    clouds = [((torch.rand((n, 5), generator=g, dtype=torch.float64) - 0.5) * 4.0).to(dtype) for n in lens]
    pad = torch.zeros((4, max(lens), 5), dtype=dtype)
    for b, c in enumerate(clouds):
        pad[b, :lens[b]] = c
        pad[b, lens[b]:] = float("nan") if b % 2 else 1e30    # whatever the padding holds
    kw = dict(origin=[0.1, 0.2, 0.3], min_points=2, return_counts=True, return_inverse=True)
    out_p = voxel_downsample(pad.cuda(), 0.3, rows=torch.tensor(lens), **kw)
    out_l = voxel_downsample([c.cuda() for c in clouds], 0.3, **kw)
    out_c = voxel_downsample(pad, 0.3, rows=lens, **kw)
    assert all(t.device.type == "cpu" for t in out_c)
    for a, b_ in zip(out_p, out_c):
        assert torch.equal(a.cpu(), b_)
    for b, c in enumerate(clouds):
        r = int(out_p[1][b])
        sep = voxel_downsample(c.cuda(), 0.3, **kw)
        one_cpu = voxel_downsample(c, 0.3, **kw)
        assert sep[0].shape == (r, 5) and sep[1].dim() == 0 and int(sep[1]) == r and sep[2].shape == (r,) and sep[3].shape == (lens[b],)
        assert one_cpu[0].device.type == "cpu"
        for i, want in enumerate((out_p[0][b, :r], out_p[1][b], out_p[2][b, :r], out_p[3][b, :lens[b]])):
            assert torch.equal(sep[i], want) and torch.equal(out_l[i][b], want) and torch.equal(one_cpu[i], want.cpu())


@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_reproducible(dtype):
    pts = _uniform(8, 60000, 6, dtype, seed=41, scale=3.0)
    pts[0, :20000, :3] = 0.5                                   # a 20000-row voxel: the block reduction
    runs = []
    for _ in range(2):
        x = pts.cuda().requires_grad_(True)
        cent, ro = voxel_downsample(x, 0.2, min_points=2)
        g = torch.cos(torch.arange(cent.numel(), device="cuda", dtype=dtype)).view_as(cent)
        (cent * g).sum().backward()
        runs.append((cent.detach().cpu(), ro.cpu(), x.grad.cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b) if not a.is_floating_point() else torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_gradcheck_float64():
    g = torch.Generator().manual_seed(2)
    pts = torch.rand((2, 60, 4), generator=g, dtype=torch.float64)
    x = pts.cuda().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: voxel_downsample(t, 0.4, min_points=2)[0], (x,), eps=1e-6, atol=1e-9, rtol=1e-7)


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_is_exactly_the_gather_divide(dtype):
    pts = _uniform(3, 20000, 4, dtype, seed=43)
    pts[1, 50:60] = float("nan")
    rows = [20000, 15000, 9000]
    x = pts.cuda().requires_grad_(True)
    cent, ro, cnt, inv = voxel_downsample(x, 0.3, rows=torch.tensor(rows), min_points=3, return_counts=True, return_inverse=True)
    gc = torch.randn(cent.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dtype)
    (cent * gc.cuda()).sum().backward()
    got = x.grad.cpu().numpy()
    gn, cn, iv = gc.numpy(), cnt.cpu().numpy(), inv.cpu().numpy()
    for b in range(3):
        want = np.zeros_like(got[b])
        on = iv[b] >= 0
        want[on] = gn[b][iv[b][on]] / cn[b][iv[b][on]].astype(gn.dtype)[:, None]
        assert np.array_equal(got[b], want)


def _chain(src_raw, tgt_raw, size, mean_of, K=4):
    """raw source / target points -> centroids (mean_of) -> normals -> pt2pl ICP; -> (T, grad src_raw, grad tgt_raw)"""
    s = src_raw.clone().cuda().requires_grad_(True)
    t = tgt_raw.clone().cuda().requires_grad_(True)
    cs, rs = mean_of(s, size)
    ct, rt = mean_of(t, size)
    assert int(rs.min()) >= 1 and int(rt.min()) >= 1 and int(rs.max()) <= cs.shape[1] and int(rt.max()) <= ct.shape[1]
    nrm = estimate_normals(ct, k=12, rows=rt)
    icp = ICP(icp_type="pt2pl", differentiable=True, max_iterations=K, tolerance=1e-12)
    icp.const_iter = True
    T0 = torch.eye(4, dtype=src_raw.dtype).repeat(src_raw.shape[0], 1, 1).cuda()
    out = icp.icp(cs, torch.cat((ct, nrm), -1), T0, trim_dist=2.0, loss_fn={"name": "huber", "metric": 1.0}, source_rows=rs, target_rows=rt)
    out["T"][:, :3].sum().backward()
    return out["T"].detach().cpu(), s.grad.cpu(), t.grad.cpu()


def _torch_mean(x, size):
    """the same centroids by a float64 index_add_ mean on the oracle's inverse (torch autograd all the way)"""
    N, m, c = x.shape
    cents, rows = [], []
    for b in range(N):
        _, cnt, inv, _ = _oracle(x[b].detach().cpu().numpy(), size, None, 1)
        inv_t = torch.tensor(inv, device=x.device)
        V = cnt.shape[0]
        on = inv_t >= 0
        s = torch.zeros((V, c), dtype=torch.float64, device=x.device).index_add_(0, inv_t[on], x[b][on].double())
        cents.append((s / torch.tensor(cnt, dtype=torch.float64, device=x.device)[:, None]).to(x.dtype))
        rows.append(V)
    M = max(rows)
    out = torch.stack([torch.cat((cb, cb.new_zeros((M - cb.shape[0], c)))) for cb in cents])
    return out, torch.tensor(rows, dtype=torch.int32, device=x.device)


@pytest.mark.parametrize("dtype", DTYPES)
def test_composition_with_normals_and_icp(dtype):
    src, tgt = make_scene_pairs(4, 12000, 16000, seed=6, dtype=dtype)
    src_raw, tgt_raw = src.contiguous(), tgt[..., :3].contiguous()
    size = 0.3
    T1, gs1, gt1 = _chain(src_raw, tgt_raw, size, lambda x, s: voxel_downsample(x, s))
    T2, gs2, gt2 = _chain(src_raw, tgt_raw, size, _torch_mean)
    assert float((T1 - T2).abs().max()) <= 2e-5
    for got, want in ((gs1, gs2), (gt1, gt2)):
        assert torch.isfinite(got).all() and float(got.abs().max()) > 0
        for b in range(got.shape[0]):
            assert float((got[b] - want[b]).abs().max()) <= 2e-4 * max(1e-6, float(want[b].abs().max())), b
