"""estimate_normals on the MI355X against its definition (dicp_amd/normals.py): neighbours index for index against a numpy brute force that
computes d2 with the same statements, normals / curvature against float64 numpy on those neighbourhoods, the scene generator's own normals,
gradients against autograd, and the plumbing (CPU tensors, lists, padded rows)."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.normals import estimate_normals
from dicp_amd.synthetic import make_pairs, make_scene_pairs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import walk_layouts as wl  # noqa: E402

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


def _autograd_oracle(P, nbr, vp, gn, gc=None):
    """dL/dP of L = sum gn . n (+ sum gc curvature) through torch.linalg.eigh in float64 on the given neighbourhoods (the sign taken from the
    forward)"""
    p = torch.tensor(P, dtype=torch.float64, requires_grad=True)
    idx = torch.tensor(nbr)
    q = p[idx] - p[:, None, :]
    d = q - q.mean(1, keepdim=True)
    C = d.transpose(1, 2) @ d / idx.shape[1]
    w, V = torch.linalg.eigh(C)
    v0 = V[:, :, 0]
    s = torch.where(((torch.tensor(vp)[None] - p.detach()) * v0.detach()).sum(1) < 0, -1.0, 1.0).to(torch.float64)
    L = (gn * (s[:, None] * v0)).sum()
    if gc is not None:
        L = L + (gc * w[:, 0] / w.sum(1)).sum()
    L.backward()
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


# ---------------------------------------------------------------- neighbour lists that leave the LDS windows (tests/walk_layouts.py)
#
# The layouts `wall` (20000 rows, x in +-1e-3) and `cube` (40000 uniform rows) put 83-88 % and 18-47 % of the backward's (query, neighbour)
# entries outside the block's window (csrc/normals.hip: global atomics instead of LDS atomics); every case asserts that share with the numpy
# window model on the brute force's lists before it looks at a GPU result.

WALK_DTYPES = [torch.float32, torch.float64]
WALK_IDS = ["f32", "f64"]
WALK_VP = np.array([5.0, 0.3, -0.2])                         # in front of the wall: its normals are +x there


@functools.lru_cache(maxsize=None)
def _walk_case(name, dtype):
    """-> (points in the dtype, k, the brute force's neighbour lists, the window model on them), the layout's condition asserted"""
    P, k = wl.normals_layout(name)
    P = P.astype(wl.np_dtype(dtype))
    ref = _knn_oracle(P, k)
    w = wl.normals_windows(P, k, dtype, ref)
    print("normals %s %s: backward entries outside the window %.3f, max in-degree %d" % (name, P.dtype.name, w.share(), w.indegree.max()))
    wl.check_normals_conditions(name, dtype, w)
    return P, k, ref, w


@pytest.mark.parametrize("dtype", WALK_DTYPES, ids=WALK_IDS)
def test_walk_neighbours_exact_on_the_wall(dtype):
    P, k, ref, _ = _walk_case("wall", dtype)
    nbr = estimate_normals(torch.from_numpy(P).cuda(), k=k, return_neighbors=True)[1].cpu().numpy()
    assert np.array_equal(nbr, ref), "%d rows differ" % int((nbr != ref).any(1).sum())


def _walk_batch(dtype):
    """N = 3: wall, cube and a ragged cloud, padded to 40000 rows with points that would be neighbours if a row count were ignored"""
    dt = wl.np_dtype(dtype)
    Pw, k, ref_w, _ = _walk_case("wall", dtype)
    Pc, _, ref_c, _ = _walk_case("cube", dtype)
    rows = [Pw.shape[0], Pc.shape[0], 12345]
    pts = np.stack([wl.wall(40000, 31), wl.cube(40000, 32), wl.cube(40000, 33)]).astype(dt)
    pts[0, :rows[0]], pts[1] = Pw, Pc
    return pts, rows, k, [ref_w, ref_c, None]


@pytest.mark.parametrize("dtype", WALK_DTYPES, ids=WALK_IDS)
def test_walk_neighbours_exact_in_a_ragged_batch(dtype):
    pts, rows, k, refs = _walk_batch(dtype)
    nbr = estimate_normals(torch.from_numpy(pts).cuda(), k=k, rows=torch.tensor(rows, dtype=torch.int32).cuda(), return_neighbors=True)[1].cpu().numpy()
    for b in range(3):
        ref = refs[b] if refs[b] is not None else _knn_oracle(pts[b, :rows[b]], k)
        assert np.array_equal(nbr[b, :rows[b]], ref), "cloud %d: %d rows differ" % (b, int((nbr[b, :rows[b]] != ref).any(1).sum()))
        assert np.all(nbr[b, rows[b]:] == -1)


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 1e-4)], ids=["f64", "f32"])
def test_walk_normals_match_oracle_on_the_wall(dtype, tol):
    P, k, ref, _ = _walk_case("wall", dtype)
    nrm, curv, nbr = estimate_normals(torch.from_numpy(P).cuda(), k=k, viewpoint=torch.tensor(WALK_VP, dtype=dtype), return_curvature=True,
                                      return_neighbors=True)
    nrm, curv, nbr = nrm.cpu().numpy().astype(np.float64), curv.cpu().numpy(), nbr.cpu().numpy()
    assert np.array_equal(nbr, ref)
    n_ref, c_ref, gap = _normals_oracle(P, nbr, WALK_VP)
    assert gap.min() > 1e-3                                  # a wall: every normal is well defined
    ang = np.linalg.norm(np.cross(nrm, n_ref), axis=1) / np.linalg.norm(nrm, axis=1)
    assert ang.max() <= tol
    assert np.all(np.einsum("ma,ma->m", nrm, n_ref) > 0)
    assert np.all(n_ref[:, 0] > 0.9) and np.all(nrm[:, 0] > 0.9)         # +x, towards the viewpoint
    np.testing.assert_allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-6 if dtype == torch.float32 else 1e-12)
    np.testing.assert_allclose(curv, c_ref, rtol=1e-4 if dtype == torch.float32 else 1e-9, atol=1e-6 if dtype == torch.float32 else 1e-13)


# The bars of the gradient tests below are the existing ones: float32 |got - ref| / |ref| < 1e-3 per cloud (test_gradient_float32_against_float64_oracle),
# float64 1e-9 (test_gradient_through_pt2pl_icp).  The reference is float64 autograd through torch.linalg.eigh on the kernel's neighbourhoods; the
# closed form of walk_layouts.normals_grad_closed_form is a second evaluation of it, and the tests print the two references' disagreement.
# (Float64, on the host: the two references differ by 6e-16 of the gradient's norm on wall and 3e-15 on cube, six orders under the float64 bar.)
WALK_BAR = {torch.float32: 1e-3, torch.float64: 1e-9}
GAP_MIN = 1e-2                                               # g is zeroed where (lam1 - lam0) / trace of the reference is below this


def _walk_upstream(P, nbr, seed):
    """random g_nrm (m,3) and g_curv (m,) in float64, zero on the rows whose reference eigen gap is below GAP_MIN (at most 5 % of them)"""
    rng = np.random.default_rng(seed)
    m = P.shape[0]
    gn, gc = rng.standard_normal((m, 3)), rng.standard_normal(m)
    gap = _normals_oracle(P, nbr, WALK_VP)[2]
    low = gap < GAP_MIN
    assert low.mean() <= 0.05, low.mean()
    gn[low], gc[low] = 0.0, 0.0
    return gn, gc


def _walk_backward(pts, k, gn, gc, dtype, rows=None):
    """estimate_normals forward + backward on the GPU with both upstream gradients -> (neighbours, points' gradient) as numpy"""
    x = torch.from_numpy(pts).cuda().requires_grad_(True)
    nrm, curv, nbr = estimate_normals(x, k=k, viewpoint=torch.tensor(WALK_VP, dtype=dtype), rows=rows, return_curvature=True, return_neighbors=True)
    torch.autograd.backward([nrm, curv], [torch.from_numpy(gn).to(dtype).cuda(), torch.from_numpy(gc).to(dtype).cuda()])
    return nbr.cpu().numpy(), x.grad.cpu().numpy()


@pytest.mark.parametrize("dtype", WALK_DTYPES, ids=WALK_IDS)
@pytest.mark.parametrize("name", wl.NORMALS_LAYOUTS)
def test_walk_gradient_against_float64_oracle(name, dtype):
    P, k, ref_nbr, w = _walk_case(name, dtype)
    dt = wl.np_dtype(dtype)
    gn, gc = _walk_upstream(P, ref_nbr, 41)
    gn, gc = gn.astype(dt).astype(np.float64), gc.astype(dt).astype(np.float64)      # (what the kernel is given, exactly)
    nbr, got = _walk_backward(P, k, gn, gc, dtype)
    assert np.array_equal(nbr, ref_nbr)
    ref = _autograd_oracle(P.astype(np.float64), nbr, WALK_VP, torch.from_numpy(gn), torch.from_numpy(gc))
    c, ref2 = wl.normals_grad_closed_form(P, nbr, WALK_VP, gn, gc)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print("normals %s %s: |got - autograd| / |autograd| = %.3e, |closed form - autograd| / |autograd| = %.3e"
          % (name, dt.name, err, np.linalg.norm(ref2 - ref) / np.linalg.norm(ref)))
    assert err < WALK_BAR[dtype], err

    # The eigen part of the backward is per query and the scatter is linear: the gradient for g on the half of the queries with the most
    # entries outside the window plus the gradient for g on the other half is the gradient for all of g, up to the order of the sums.  Row l
    # with in-degree D_l: (D_l + 2) u_T sum |contribution| over its entries.  The kernel does not expose its per-entry contributions, and the
    # two partial gradients only give |sum| <= sum |.|, so sum |contribution| is taken from the closed form on the same neighbourhoods (float64,
    # within 1e-14 of the kernel's terms).  Each term is rounded to T identically in all three runs, so only the additions differ: the strict
    # worst case over three sums in unspecified orders is (D - 1) + (D_a - 1) + (D_b - 1) = (2 D - 3) u_T sum |contribution|, above D + 2 for
    # D > 5.  The bar stays at the D + 2 this check was specified with: rounding errors of the additions do not align, a row's error grows like
    # sqrt(D) u_T, and the worst ratio printed below is the margin actually seen.
    out = w.bwd_outside.sum(1)
    order = np.argsort(-out, kind="stable")
    half = np.zeros(P.shape[0], bool)
    half[order[:P.shape[0] // 2]] = True
    assert out[half].sum() >= 0.5 * out.sum() and out[half].sum() > 0
    parts = []
    for sel in (half, ~half):
        parts.append(_walk_backward(P, k, np.where(sel[:, None], gn, 0.0), np.where(sel, gc, 0.0), dtype)[1].astype(np.float64))
    A = np.zeros((P.shape[0], 3))
    for a in range(3):
        A[:, a] = np.bincount(nbr.reshape(-1), weights=np.abs(c[:, :, a]).reshape(-1), minlength=P.shape[0])
    bound = ((w.indegree + 2) * wl.U[dt])[:, None] * A
    r = wl.assert_within(got, parts[0] + parts[1], bound, "normals %s: halves against the whole" % name)
    print("normals %s %s: halves against the whole, worst error / bound %.3f" % (name, dt.name, r))


@pytest.mark.parametrize("dtype", WALK_DTYPES, ids=WALK_IDS)
def test_walk_gradient_in_a_ragged_batch_against_single_calls(dtype):
    pts, rows, k, _ = _walk_batch(dtype)
    dt = wl.np_dtype(dtype)
    ups = []
    for b in range(3):
        nb = estimate_normals(torch.from_numpy(pts[b, :rows[b]]).cuda(), k=k, return_neighbors=True)[1].cpu().numpy()
        gn, gc = _walk_upstream(pts[b, :rows[b]], nb, 50 + b)
        ups.append((gn.astype(dt).astype(np.float64), gc.astype(dt).astype(np.float64)))
    gn, gc = np.random.default_rng(60).standard_normal((3, 40000, 3)), np.random.default_rng(61).standard_normal((3, 40000))   # (pad rows: ignored)
    for b in range(3):
        gn[b, :rows[b]], gc[b, :rows[b]] = ups[b]
    _, got = _walk_backward(pts, k, gn, gc, dtype, rows=torch.tensor(rows))
    for b in range(3):
        _, one = _walk_backward(pts[b, :rows[b]], k, ups[b][0], ups[b][1], dtype)
        err = np.linalg.norm(got[b, :rows[b]].astype(np.float64) - one) / np.linalg.norm(one)
        print("normals batch cloud %d %s: |batch - single| / |single| = %.3e" % (b, dt.name, err))
        assert err < WALK_BAR[dtype], err
        assert np.all(got[b, rows[b]:] == 0)
