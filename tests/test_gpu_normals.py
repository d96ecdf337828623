"""estimate_normals on the MI355X against its definition (dicp_amd/normals.py): neighbours index for index against a numpy brute force that
computes d2 with the same statements, normals / curvature against float64 numpy on those neighbourhoods, the scene generator's own normals,
gradients against autograd, and the plumbing (CPU tensors, lists, padded rows)."""
import math

import numpy as np
import pytest
import torch

from dicp_amd.normals import estimate_normals
from dicp_amd.synthetic import make_pairs, make_scene_pairs

pytestmark = pytest.mark.gpu


def _knn_oracle(P, k, chunk=256):
    """(m,3) numpy array in its own dtype -> (m,k) int64: the k_eff = min(k, m) rows first in (d2, index) order, -1 beyond"""
    m = P.shape[0]
    ke = min(k, m)
    out = np.full((m, k), -1, dtype=np.int64)
    for a in range(0, m, chunk):
        Q = P[a:a + chunk]
        dx = P[None, :, 0] - Q[:, None, 0]
        dy = P[None, :, 1] - Q[:, None, 1]
        dz = P[None, :, 2] - Q[:, None, 2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        d2 = (xx + yy) + zz
        if ke < m:
            kth = np.partition(d2, ke - 1, axis=1)[:, ke - 1]
        else:
            kth = np.full(Q.shape[0], np.inf, dtype=d2.dtype)
        for r in range(Q.shape[0]):
            cand = np.flatnonzero(d2[r] <= kth[r]) if ke < m else np.arange(m)
            order = np.lexsort((cand, d2[r, cand]))          # by d2, then by index
            out[a + r, :ke] = cand[order[:ke]]
    return out


def _check_neighbours(pts, k, rows=None):
    """pts (N,m,3) torch CPU; compares every cloud's neighbour lists with the oracle's"""
    nbr = estimate_normals(pts.cuda(), k=k, rows=None if rows is None else torch.tensor(rows, dtype=torch.int32).cuda(),
                           return_neighbors=True)[1].cpu().numpy()
    N, m = pts.shape[:2]
    for b in range(N):
        mb = m if rows is None else rows[b]
        if mb > 0:
            ref = _knn_oracle(pts[b, :mb].numpy(), k)
            assert np.array_equal(nbr[b, :mb], ref), "cloud %d: %d rows differ" % (b, int((nbr[b, :mb] != ref).any(1).sum()))
        assert np.all(nbr[b, mb:] == -1)


def _cloud(N, m, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((N, m, 3), generator=g, dtype=torch.float64) * scale).to(dtype)


SMALL = [(m, k, dt) for m in (1, 2, 3, 5, 17, 1000, 2049) for k, dt in zip((3, 8, 16, 17, 32), (torch.float32, torch.float64) * 3)]


@pytest.mark.parametrize("m,k,dtype", SMALL)
def test_neighbours_exact_small(m, k, dtype):
    _check_neighbours(_cloud(3, m, dtype, seed=m * 100 + k), k)


@pytest.mark.parametrize("m,k,dtype", [(16384, 16, torch.float32), (16384, 32, torch.float64), (16385, 17, torch.float32), (40000, 8, torch.float64)])
def test_neighbours_exact_large(m, k, dtype):
    _check_neighbours(_cloud(1, m, dtype, seed=m + k, scale=10.0), k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("m,k", [(1000, 8), (20000, 16)])
def test_neighbours_ragged(dtype, m, k):
    rows = [m, k - 2, 0, m // 3]
    _check_neighbours(_cloud(4, m, dtype, seed=11 + m), k, rows=rows)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_neighbours_duplicates(dtype):
    g = torch.Generator().manual_seed(5)
    pts = (torch.randint(0, 6, (2, 3000, 3), generator=g).to(torch.float64) * 0.25).to(dtype)     # 216 distinct points, ~14 copies each
    _check_neighbours(pts, 16)
    _check_neighbours(pts, 32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_neighbours_one_x(dtype):
    pts = _cloud(2, 3000, torch.float64, seed=9)
    pts[..., 0] = 0.75
    _check_neighbours(pts.to(dtype), 16)


def test_neighbours_far_from_origin_float32():
    pts = _cloud(2, 5000, torch.float64, seed=13, scale=5.0) + torch.tensor([2500.0, -1800.0, 300.0], dtype=torch.float64)
    _check_neighbours(pts.to(torch.float32), 16)


def _normals_oracle(P, nbr, vp):
    """float64 numpy: normals, curvature, eigen gap (lam1 - lam0) / trace on the given neighbourhoods"""
    P = P.astype(np.float64)
    q = P[nbr] - P[:, None, :]
    d = q - q.mean(1, keepdims=True)
    C = np.einsum("mka,mkb->mab", d, d) / nbr.shape[1]
    w, V = np.linalg.eigh(C)
    n = V[:, :, 0]
    dot = np.einsum("ma,ma->m", n, vp[None, :] - P)
    n = n * np.where(dot < 0, -1.0, 1.0)[:, None]
    tr = w.sum(1)
    return n, np.where(tr > 0, w[:, 0] / np.where(tr > 0, tr, 1), 0.0), (w[:, 1] - w[:, 0]) / np.where(tr > 0, tr, 1)


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 1e-4)])
def test_normals_match_oracle(dtype, tol):
    pts = _cloud(2, 4000, dtype, seed=21, scale=4.0)
    pts[..., 2] = pts[..., 2] * 0.2 + 0.3 * torch.sin(pts[..., 0].to(torch.float64)).to(dtype)     # a wavy sheet: mostly clear gaps
    vp = np.array([1.0, -2.0, 5.0])
    nrm, curv, nbr = estimate_normals(pts.cuda(), k=16, viewpoint=torch.tensor(vp, dtype=dtype), return_curvature=True, return_neighbors=True)
    nrm, curv, nbr = nrm.cpu().numpy().astype(np.float64), curv.cpu().numpy(), nbr.cpu().numpy()
    for b in range(2):
        n_ref, c_ref, gap = _normals_oracle(pts[b].numpy(), nbr[b], vp)
        ok = gap > 1e-3
        assert ok.mean() > 0.95
        ang = np.linalg.norm(np.cross(nrm[b], n_ref), axis=1) / np.linalg.norm(nrm[b], axis=1)     # sin of the angle (arccos near 1 is all rounding)
        assert ang[ok].max() <= tol
        assert np.array_equal(np.sign(np.einsum("ma,ma->m", nrm[b], n_ref))[ok], np.ones(ok.sum()))
        np.testing.assert_allclose(np.linalg.norm(nrm[b], axis=1), 1.0, atol=1e-6 if dtype == torch.float32 else 1e-12)
        np.testing.assert_allclose(curv[b], c_ref, rtol=1e-4 if dtype == torch.float32 else 1e-9, atol=1e-6 if dtype == torch.float32 else 1e-13)


def test_normals_match_scene_ground_truth():
    _, tgt = make_scene_pairs(2, 16, 16384, seed=4, dtype=torch.float32, clutter=0.0)
    nrm = estimate_normals(tgt[..., :3].cuda(), k=16, viewpoint=torch.tensor([0.0, 0.0, 1.5])).cpu()
    cos = (nrm * tgt[..., 3:]).sum(-1)
    within = (cos > math.cos(math.radians(5.0))).double().mean().item()
    same = (cos > 0).double().mean().item()
    assert within >= 0.88, within
    assert same >= 0.999, same


def test_gradcheck_float64():
    g = torch.Generator().manual_seed(2)
    pts = torch.rand((2, 40, 4), generator=g, dtype=torch.float64)
    pts[..., 2] *= 0.3
    x = pts.cuda().requires_grad_(True)
    f = lambda t: estimate_normals(t, k=8, viewpoint=torch.tensor([0.5, 0.5, 3.0], dtype=torch.float64), return_curvature=True)   # noqa: E731
    assert torch.autograd.gradcheck(f, (x,), eps=1e-6, atol=1e-6, rtol=1e-4)


def _autograd_oracle(P, nbr, vp, gn):
    """dL/dP of L = sum gn . n through torch.linalg.eigh in float64 on the given neighbourhoods (the sign taken from the forward)"""
    p = torch.tensor(P, dtype=torch.float64, requires_grad=True)
    idx = torch.tensor(nbr)
    q = p[idx] - p[:, None, :]
    d = q - q.mean(1, keepdim=True)
    C = d.transpose(1, 2) @ d / idx.shape[1]
    w, V = torch.linalg.eigh(C)
    v0 = V[:, :, 0]
    s = torch.where(((torch.tensor(vp)[None] - p.detach()) * v0.detach()).sum(1) < 0, -1.0, 1.0).to(torch.float64)
    (gn * (s[:, None] * v0)).sum().backward()
    return p.grad.numpy()


def test_gradient_float32_against_float64_oracle():
    N, m = 4, 16384
    g = torch.Generator().manual_seed(8)
    xy = torch.rand((N, m, 2), generator=g, dtype=torch.float64) * 8.0
    z = 0.4 * torch.sin(xy[..., :1]) * torch.cos(0.5 * xy[..., 1:]) + 0.002 * torch.randn((N, m, 1), generator=g, dtype=torch.float64)
    pts = torch.cat((xy, z), -1).to(torch.float32)
    gn = torch.randn((N, m, 3), generator=g, dtype=torch.float64)
    x = pts.cuda().requires_grad_(True)
    vp = np.array([4.0, 4.0, 10.0])
    nrm, nbr = estimate_normals(x, k=16, viewpoint=torch.tensor(vp, dtype=torch.float32), return_neighbors=True)
    (nrm * gn.to(torch.float32).cuda()).sum().backward()
    got = x.grad.cpu().numpy().astype(np.float64)
    for b in range(N):
        ref = _autograd_oracle(pts[b].numpy().astype(np.float64), nbr[b].cpu().numpy(), vp, gn[b])
        err = np.linalg.norm(got[b] - ref) / np.linalg.norm(ref)
        assert err < 1e-3, err


def test_gradient_through_pt2pl_icp():
    from dicp_amd.ICP import ICP
    src, tgt = make_pairs(2, 600, 800, seed=3, dtype=torch.float64)
    pts = tgt[..., :3].contiguous()
    pts[..., 2] = 0.3 * torch.sin(pts[..., 0]) * 0.5 + 0.05 * pts[..., 2]      # a smooth surface, so that the normals are well defined
    T0 = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1).cuda()
    kw = dict(trim_dist=5.0, dim=3)
    s = src.cuda()

    def run(target):
        icp = ICP(icp_type="pt2pl", differentiable=True, max_iterations=3, tolerance=1e-12)
        icp.const_iter = True
        return icp.icp(s, target, T0, **kw)["T"]

    p1 = pts.cuda().requires_grad_(True)
    n1 = estimate_normals(p1, k=12)
    T1 = run(torch.cat((p1, n1), -1))
    gT = torch.randn_like(T1)
    (T1 * gT).sum().backward()

    p2 = pts.cuda().requires_grad_(True)
    n2 = estimate_normals(p2, k=12).detach().requires_grad_(True)
    T2 = run(torch.cat((p2, n2), -1))
    torch.testing.assert_close(T2, T1.detach(), rtol=0, atol=0)
    (T2 * gT).sum().backward()
    p3 = pts.cuda().requires_grad_(True)
    vjp = torch.autograd.grad(estimate_normals(p3, k=12), p3, n2.grad)[0]
    torch.testing.assert_close(p1.grad, p2.grad + vjp, rtol=1e-9, atol=1e-10)


def test_cpu_in_cpu_out():
    pts = _cloud(2, 500, torch.float32, seed=1)
    nrm, curv = estimate_normals(pts, k=8, return_curvature=True)
    assert nrm.device.type == "cpu" and curv.device.type == "cpu" and nrm.dtype == torch.float32
    ref = estimate_normals(pts.cuda(), k=8)
    assert torch.equal(nrm, ref.cpu())
    one = estimate_normals(pts[0], k=8)
    assert one.shape == (500, 3) and torch.equal(one, nrm[0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_list_padded_and_separate_agree(dtype):
    lens = [700, 40, 2, 1500]
    g = torch.Generator().manual_seed(17)
    clouds = [torch.rand((n, 5), generator=g, dtype=torch.float64).to(dtype).cuda() for n in lens]
    out_l = estimate_normals(clouds, k=16, return_curvature=True, return_neighbors=True)
    pad = torch.zeros((4, max(lens), 5), dtype=dtype).cuda()
    for b, c in enumerate(clouds):
        pad[b, :lens[b]] = c
    pad[1, 40:] = 1e6                                        # whatever the padding holds
    out_p = estimate_normals(pad, k=16, rows=torch.tensor(lens), return_curvature=True, return_neighbors=True)
    for b, c in enumerate(clouds):
        sep = estimate_normals(c, k=16, return_curvature=True, return_neighbors=True)
        for i in range(3):
            assert torch.equal(out_l[i][b], sep[i])
            assert torch.equal(out_p[i][b, :lens[b]], sep[i])
        assert torch.all(out_p[0][b, lens[b]:] == 0) and torch.all(out_p[1][b, lens[b]:] == 0) and torch.all(out_p[2][b, lens[b]:] == -1)
    assert torch.all(out_l[0][2] == 0) and torch.all(out_l[2][2][:, 2:] == -1)       # k_eff = 2 < 3: zero normals
    x = pad.clone().requires_grad_(True)
    estimate_normals(x, k=16, rows=torch.tensor(lens)).sum().backward()
    for b in range(4):
        assert torch.all(x.grad[b, lens[b]:] == 0)
    assert torch.all(x.grad[..., 3:] == 0)
