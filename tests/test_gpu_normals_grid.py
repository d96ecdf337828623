"""estimate_normals(method="grid") on the MI355X: neighbour lists index for index against the numpy brute force and normals / curvature
bit for bit against method="walk" on every cloud the walk defines (small clouds, the layouts of the grid k-NN tests, a cloud of many sort
chunks, ragged batches and every input form); the knn_points rule where rows are non-finite or d2 overflows; the device grid's order and
the scan's counters against the host build of the same header; the gradients against autograd, against the walk's, and on layouts whose
entries leave the backward's LDS window in grid order (tests/normals_grid_model.py); the zero-gradient rules; pt2pl ICP; no host
synchronisation; graph capture."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.ball import CellGrid
from dicp_amd.normals import estimate_normals

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ball_clouds as bc  # noqa: E402
import gridknn_host as gh  # noqa: E402
import normals_grid_model as ng  # noqa: E402
import walk_layouts as wl  # noqa: E402
from test_gpu_normals import (SMALL, WALK_BAR, WALK_VP, _autograd_oracle, _cloud, _knn_oracle, _walk_case,  # noqa: E402
                              _walk_upstream)

pytestmark = pytest.mark.gpu

TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
VP = np.array([1.0, -2.0, 5.0])


def _run(pts, k, method, **kw):
    """-> (normals, curvature, neighbours) as numpy"""
    outs = estimate_normals(pts, k=k, return_curvature=True, return_neighbors=True, method=method, **kw)
    return tuple(o.detach().cpu().numpy() for o in outs)


def _same_bits(a, b, what):
    for x, y, name in zip(a, b, ("normals", "curvature", "neighbours")):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, name)
        if x.tobytes() != y.tobytes():
            rows = np.flatnonzero((x.reshape(-1, x.shape[-1] if name != "curvature" else 1).view(np.uint8)
                                   != y.reshape(-1, y.shape[-1] if name != "curvature" else 1).view(np.uint8)).any(1))
            raise AssertionError("%s: %s differ from the walk's in %d rows, first %d" % (what, name, rows.size, rows[0]))


def _hold(P, k, what=""):
    """one finite cloud (m,3) numpy: the grid against the brute force and, bit for bit, against the walk"""
    x = torch.from_numpy(np.array(P)).cuda()
    vp = torch.tensor(VP, dtype=x.dtype)
    grid = _run(x, k, "grid", viewpoint=vp)
    ref = _knn_oracle(P, k)
    assert np.array_equal(grid[2], ref), "%s k=%d: %d rows differ from the brute force" % (what, k, int((grid[2] != ref).any(1).sum()))
    _same_bits(grid, _run(x, k, "walk", viewpoint=vp), "%s k=%d" % (what, k))
    return grid


# ------------------------------------------------------------------ 1. small clouds
@pytest.mark.parametrize("m,k,dtype", SMALL)
def test_small_clouds(m, k, dtype):
    pts = _cloud(3, m, dtype, seed=m * 100 + k)
    x = pts.cuda()
    grid = _run(x, k, "grid")
    for b in range(3):
        assert np.array_equal(grid[2][b], _knn_oracle(pts[b].numpy(), k)), b
    _same_bits(grid, _run(x, k, "walk"), "m=%d k=%d" % (m, k))
    assert (np.abs(np.linalg.norm(grid[0], axis=-1) - 1.0) < 1e-5).all() == (m >= 3)


# ------------------------------------------------------------------ 2. the layouts of the grid k-NN tests, non-finite rows, overflow
def _fit_by_rule(P, nbr, vp):
    """numpy restatement in float64 of the definition with a k_eff per row: -> normals (m,3), curvature (m,), gap (m,); zero for k_eff < 3"""
    m = P.shape[0]
    P64 = P.astype(np.float64)
    n, c, gap = np.zeros((m, 3)), np.zeros(m), np.zeros(m)
    ke = (nbr >= 0).sum(1)
    for i in np.flatnonzero(ke >= 3):
        q = P64[nbr[i, :ke[i]]] - P64[i]
        d = q - q.mean(0)
        w, V = np.linalg.eigh(d.T @ d / ke[i])
        v = V[:, 0] * (-1.0 if V[:, 0] @ (vp - P64[i]) < 0 else 1.0)
        tr = w.sum()
        n[i], c[i], gap[i] = v, (w[0] / tr if tr > 0 else 0.0), ((w[1] - w[0]) / tr if tr > 0 else 0.0)
    return n, c, gap


def _hold_rule(P, k, what):
    """a cloud with non-finite rows or d2 that overflow: the knn_points rule"""
    dt = P.dtype
    x = torch.from_numpy(np.array(P)).cuda()
    nrm, curv, nbr = _run(x, k, "grid", viewpoint=torch.tensor(VP, dtype=x.dtype))
    ref = wl.knn_oracle(P, P, k)[1]                         # candidates: finite d2 only; a non-finite row has none and is nobody's
    assert np.array_equal(nbr, ref), "%s k=%d: %d rows differ from the rule's lists" % (what, k, int((nbr != ref).any(1).sum()))
    bad = ~np.isfinite(P).all(1)
    assert (nbr[bad] == -1).all() and not np.isin(nbr, np.flatnonzero(bad)).any()
    ke = (ref >= 0).sum(1)
    assert (nrm[ke < 3] == 0).all() and (curv[ke < 3] == 0).all() and np.isfinite(nrm).all() and np.isfinite(curv).all()
    n_ref, c_ref, gap = _fit_by_rule(P, ref, VP)
    ok = (ke >= 3) & (gap > 1e-3)
    if ok.any():
        got = nrm[ok].astype(np.float64)
        ang = np.linalg.norm(np.cross(got, n_ref[ok]), axis=1)
        assert ang.max() <= (1e-4 if dt == np.float32 else 1e-10) and (np.einsum("ma,ma->m", got, n_ref[ok]) > 0).all()
    full = ke >= 3
    np.testing.assert_allclose(curv[full], c_ref[full], rtol=1e-4 if dt == np.float32 else 1e-9, atol=1e-6 if dt == np.float32 else 1e-13)
    return nrm, curv, nbr, ke


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_grid_layouts(dtype):
    names, by_rule = set(), set()
    seen = []
    for name, _, y in gh.all_cases(dtype):
        if any(y.shape == s.shape and np.array_equal(y, s, equal_nan=True) for s in seen):
            continue                                        # (the lattice at several radii: one cloud)
        seen.append(y)
        names.add(name)
        d2 = wl.knn_oracle(y, y, 32)[1]
        defined = np.isfinite(y).all() and ((d2 >= 0).sum(1) == min(32, y.shape[0])).all()
        for k in (8, 32):
            if defined:
                grid = _hold(y, k, name)
                if name == "lattice r=1.0" and k == 8:
                    assert grid[2][171, :7].tolist() == [171, 122, 164, 170, 172, 178, 220]        # six rows at d2 = 1 in six cells: by index
            else:
                by_rule.add(name)
                _hold_rule(y, k, name)
    assert {"lattice r=1.0", "300 copies", "line along z", "line along x", "wall", "two clusters", "extent 3e38"} <= names
    assert by_rule == ({"k above the live rows", "extent 3e38"} if dtype == np.float32 else {"k above the live rows"})


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_non_finite_rows(dtype):
    y = bc.nonfinite_pair(dtype)[1]
    bad = [5, 17, 400, 899]
    keep = np.setdiff1d(np.arange(y.shape[0]), bad)
    for k in (8, 32):
        nrm, curv, nbr, ke = _hold_rule(y, k, "non-finite rows")
        assert (ke[bad] == 0).all() and (ke[keep] == k).all() and (nrm[bad] == 0).all() and (nbr[bad] == -1).all()
        # the finite rows alone are a cloud the walk defines: the same bits, the indices shifted
        sub = _run(torch.from_numpy(y[keep]).cuda(), k, "walk", viewpoint=torch.tensor(VP, dtype=TORCH[np.dtype(dtype)]))
        _same_bits((nrm[keep], curv[keep], nbr[keep]), (sub[0], sub[1], keep[sub[2]]), "finite rows k=%d" % k)


# ------------------------------------------------------------------ 3. a cloud of many sort chunks
def test_large_cloud():
    """20000 rows: 32768 sorted slots, 16 LDS chunks and every stride of the sort between them"""
    _hold(_cloud(1, 20000, torch.float32, seed=20016, scale=10.0)[0].numpy(), 16, "20000 rows")


# ------------------------------------------------------------------ 4. ragged batches and input forms
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_ragged_batches(dtype):
    m, k = 1000, 8
    rows = [m, k - 2, 0, m // 3]
    pts = _cloud(4, m, dtype, seed=1011)
    singles = [_run(pts[b, :r].cuda(), k, "grid") if r else None for b, r in enumerate(rows)]
    for b, r in enumerate(rows):
        if r:
            assert np.array_equal(singles[b][2], _knn_oracle(pts[b, :r].numpy(), k))
            _same_bits(singles[b], _run(pts[b, :r].cuda(), k, "walk"), "cloud %d alone" % b)
    assert (singles[1][0] != 0).all(1).any() and (singles[1][2][:, 6:] == -1).all()     # k_eff = 6
    for fill in ("nan", "decoy"):                           # pad rows: NaN, and rows that would be neighbours if they took part
        x = pts.clone()
        for b, r in enumerate(rows):
            x[b, r:] = float("nan") if fill == "nan" else x[b, :max(r, 1)].mean(0) if r else 0.5
        for dev in ("cuda", "cpu"):
            got = _run(x.cuda(), k, "grid", rows=torch.tensor(rows, dtype=torch.int32 if dev == "cuda" else torch.int64).to(dev))
            for b, r in enumerate(rows):
                if r:
                    _same_bits(tuple(o[b, :r] for o in got), singles[b], "%s rows on %s cloud %d" % (fill, dev, b))
                assert (got[0][b, r:] == 0).all() and (got[1][b, r:] == 0).all() and (got[2][b, r:] == -1).all()
        if fill == "decoy":
            _same_bits(got, _run(x.cuda(), k, "walk", rows=torch.tensor(rows)), "the padded batch")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_lists_wide_rows_views_and_cpu_tensors(dtype):
    lens = [700, 40, 2, 1500]
    g = torch.Generator().manual_seed(17)
    clouds = [torch.rand((n, 5), generator=g, dtype=torch.float64).to(dtype).cuda() for n in lens]
    out_l = estimate_normals(clouds, k=16, return_curvature=True, return_neighbors=True, method="grid")
    walk_l = estimate_normals(clouds, k=16, return_curvature=True, return_neighbors=True)
    for b, c in enumerate(clouds):
        sep = estimate_normals(c, k=16, return_curvature=True, return_neighbors=True, method="grid")
        for i in range(3):
            assert out_l[i][b].shape[0] == lens[b] and torch.equal(out_l[i][b], sep[i]) and torch.equal(out_l[i][b], walk_l[i][b])
        assert np.array_equal(sep[2].cpu().numpy(), _knn_oracle(c[:, :3].cpu().numpy(), 16))
    assert torch.all(out_l[0][2] == 0) and torch.all(out_l[2][2][:, 2:] == -1)       # k_eff = 2 < 3: zero normals
    wide = torch.cat((clouds[0], clouds[0], clouds[0]), 1)[:, 5:9]                   # a non-contiguous view of 4 columns
    assert not wide.is_contiguous()
    assert torch.equal(estimate_normals(wide, k=16, method="grid"), out_l[0][0])
    cpu = estimate_normals(clouds[3].cpu(), k=16, return_curvature=True, method="grid")
    assert all(o.device.type == "cpu" and o.dtype == dtype for o in cpu) and torch.equal(cpu[0], out_l[0][3].cpu()) and torch.equal(cpu[1], out_l[1][3].cpu())


# ------------------------------------------------------------------ 5. / 6. the device grid and the counters against the host build
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_grid_order_equals_the_host_model(dtype):
    P = bc.random_pair(1, 5000, dtype, seed=2)[1]
    P[[7, 4100]] = np.nan
    g = ng.grid_order(P, rows=4900)
    grid = CellGrid.by_density(torch.from_numpy(P).cuda().unsqueeze(0), torch.tensor([4900], dtype=torch.int32).cuda())
    assert np.array_equal(grid.perm[0, :5000].cpu().numpy(), g.perm)
    keys = grid.keys[0].cpu().numpy().view(np.uint64)
    assert np.array_equal(keys[:5000], g.keys[g.perm]) and (keys[g.cnt:] == ng.NO_KEY).all() and g.cnt == 4898


def test_counters_equal_the_host_build():
    """the same header on the host and on the device: the same plan, the same cells, the same rows"""
    clouds = [bc.random_pair(1, 5000, np.float32, seed=s)[1] for s in (0, 1)]
    X = torch.from_numpy(np.stack(clouds)).cuda()
    for k in (8, 16, 32):
        visited = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        passes = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        estimate_normals(X, k=k, method="grid", _visited=visited, _passes=passes)
        for b, P in enumerate(clouds):
            _, st = gh.header(P, P, k)
            assert (int(visited[b]), int(passes[b])) == (st["visited"], st["passes"]), (k, b)


# ------------------------------------------------------------------ 7. gradients
def test_gradcheck_float64():
    g = torch.Generator().manual_seed(2)
    pts = torch.rand((2, 40, 4), generator=g, dtype=torch.float64)
    pts[..., 2] *= 0.3
    x = pts.cuda().requires_grad_(True)
    f = lambda t: estimate_normals(t, k=8, viewpoint=torch.tensor([0.5, 0.5, 3.0], dtype=torch.float64), return_curvature=True,   # noqa: E731
                                   method="grid")
    assert torch.autograd.gradcheck(f, (x,), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_gradient_float32_against_float64_oracle():
    N, m = 2, 4096
    g = torch.Generator().manual_seed(8)
    xy = torch.rand((N, m, 2), generator=g, dtype=torch.float64) * 4.0
    z = 0.4 * torch.sin(xy[..., :1]) * torch.cos(0.5 * xy[..., 1:]) + 0.002 * torch.randn((N, m, 1), generator=g, dtype=torch.float64)
    pts = torch.cat((xy, z), -1).to(torch.float32)
    gn = torch.randn((N, m, 3), generator=g, dtype=torch.float64)
    x = pts.cuda().requires_grad_(True)
    vp = np.array([2.0, 2.0, 10.0])
    nrm, nbr = estimate_normals(x, k=16, viewpoint=torch.tensor(vp, dtype=torch.float32), return_neighbors=True, method="grid")
    (nrm * gn.to(torch.float32).cuda()).sum().backward()
    got = x.grad.cpu().numpy().astype(np.float64)
    for b in range(N):
        ref = _autograd_oracle(pts[b].numpy().astype(np.float64), nbr[b].cpu().numpy(), vp, gn[b])
        err = np.linalg.norm(got[b] - ref) / np.linalg.norm(ref)
        print("wavy sheet cloud %d: |got - autograd| / |autograd| = %.3e" % (b, err))
        assert err < 1e-3, err


@functools.lru_cache(maxsize=None)
def _grad_case(name, dtype):
    """-> (points in the dtype, the brute force's lists, the window model on them in grid order), the layout's condition asserted"""
    P = ng.grad_layout(name, dtype)
    if name == "cube" and dtype == "float32":
        Pw, k, ref, _ = _walk_case("cube", torch.float32)   # the same cloud as the walk's test: its brute force, once per process
        assert k == ng.K_GRAD and np.array_equal(Pw, P)
    else:
        ref = _knn_oracle(P, ng.K_GRAD)
    w = ng.grid_windows(P, ng.K_GRAD, dtype, ref)
    s = ng.check_grad_conditions(name, w)
    print("normals grid %s %s: backward entries outside the window %.3f, max in-degree %d" % (name, dtype, s, w.indegree.max()))
    return P, ref, w


def _backward(P, gn, gc, method):
    dtype = TORCH[P.dtype]
    x = torch.from_numpy(P).cuda().requires_grad_(True)
    nrm, curv, nbr = estimate_normals(x, k=ng.K_GRAD, viewpoint=torch.tensor(WALK_VP, dtype=dtype), return_curvature=True, return_neighbors=True,
                                      method=method)
    torch.autograd.backward([nrm, curv], [torch.from_numpy(gn).to(dtype).cuda(), torch.from_numpy(gc).to(dtype).cuda()])
    return nbr.cpu().numpy(), x.grad.cpu().numpy()


@pytest.mark.parametrize("name,dtype", ng.GRAD_LAYOUTS)
def test_gradient_on_window_layouts(name, dtype):
    P, ref_nbr, w = _grad_case(name, dtype)
    dt = P.dtype
    bar = WALK_BAR[TORCH[dt]]
    gn, gc = _walk_upstream(P, ref_nbr, 41)
    gn, gc = gn.astype(dt).astype(np.float64), gc.astype(dt).astype(np.float64)      # (what the kernel is given, exactly)
    nbr, got = _backward(P, gn, gc, "grid")
    assert np.array_equal(nbr, ref_nbr)
    ref = _autograd_oracle(P.astype(np.float64), nbr, WALK_VP, torch.from_numpy(gn), torch.from_numpy(gc))
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    walk = _backward(P, gn, gc, "walk")[1]
    err_w = np.linalg.norm(got.astype(np.float64) - walk) / np.linalg.norm(walk)
    print("normals grid %s %s: |got - autograd| / |autograd| = %.3e, |grid - walk| / |walk| = %.3e" % (name, dt.name, err, err_w))
    assert err < bar, err
    assert err_w < bar, err_w
    if name != "cube":
        return
    # The halves of the queries, as test_gpu_normals.test_walk_gradient_against_float64_oracle has it and with its bound: the gradient for g
    # on the half of the queries with the most entries outside the window plus the gradient for g on the other half is the gradient for
    # all of g up to the order of the sums, (D_l + 2) u_T sum |contribution| for row l of in-degree D_l (the contributions from the float64
    # closed form on the same neighbourhoods).
    c, _ = wl.normals_grad_closed_form(P, nbr, WALK_VP, gn, gc)
    out = w.bwd_outside.sum(1)
    order = np.argsort(-out, kind="stable")
    half = np.zeros(P.shape[0], bool)
    half[order[:P.shape[0] // 2]] = True
    assert out[half].sum() >= 0.5 * out.sum() and out[half].sum() > 0
    parts = [_backward(P, np.where(sel[:, None], gn, 0.0), np.where(sel, gc, 0.0), "grid")[1].astype(np.float64) for sel in (half, ~half)]
    A = np.zeros((P.shape[0], 3))
    for a in range(3):
        A[:, a] = np.bincount(nbr.reshape(-1), weights=np.abs(c[:, :, a]).reshape(-1), minlength=P.shape[0])
    bound = ((w.indegree + 2) * wl.U[dt])[:, None] * A
    r = wl.assert_within(got, parts[0] + parts[1], bound, "normals grid %s: halves against the whole" % name)
    print("normals grid %s %s: halves against the whole, worst error / bound %.3f" % (name, dt.name, r))


# ------------------------------------------------------------------ 8. the zero-gradient rules
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_zero_gradient_rules(dtype):
    """NaN cotangents on pad rows, non-finite rows and zero-normal rows leave finite gradients; columns >= 3, pad rows and non-finite
    rows get exactly zero"""
    m, k = 600, 16
    g = torch.Generator().manual_seed(23)
    pts = torch.rand((3, m, 5), generator=g, dtype=torch.float64).to(dtype)
    pts[..., 2] *= 0.2
    rows = [m, 2, 350]
    pts[0, 11, 1] = float("nan")
    pts[0, 300, :3] = float("inf")
    pts[2, 350:] = float("nan")
    x = pts.cuda().requires_grad_(True)
    nrm, curv, nbr = estimate_normals(x, k=k, rows=torch.tensor(rows).cuda(), return_curvature=True, return_neighbors=True, method="grid")
    zero = (nrm == 0).all(-1)
    live = torch.zeros((3, m), dtype=torch.bool)
    for b, r in enumerate(rows):
        live[b, :r] = True
    live[0, [11, 300]] = False
    live[1] = False                                         # k_eff = 2
    assert torch.equal(zero.cpu(), ~live) and (nbr[0, [11, 300]] == -1).all() and (nbr[1, :2, :2] >= 0).all() and (nbr[1, 2:] == -1).all()
    gn = torch.where(zero[..., None], torch.full_like(nrm, float("nan")), torch.ones_like(nrm))
    gc = torch.where(zero, torch.full_like(curv, float("nan")), torch.ones_like(curv))
    torch.autograd.backward([nrm, curv], [gn, gc])
    gr = x.grad.cpu()
    assert torch.isfinite(gr).all()
    assert (gr[..., 3:] == 0).all() and (gr[1] == 0).all() and (gr[2, 350:] == 0).all() and (gr[0, [11, 300]] == 0).all()
    assert (gr[0, :, :3] != 0).any() and (gr[2, :350, :3] != 0).any()
    assert not nbr.requires_grad


# ------------------------------------------------------------------ 9. through ICP
def test_pt2pl_icp_takes_the_same_poses():
    from dicp_amd.ICP import ICP
    from dicp_amd.synthetic import make_pairs
    src, tgt = make_pairs(2, 600, 800, seed=3, dtype=torch.float64)
    pts = tgt[..., :3].contiguous()
    pts[..., 2] = 0.3 * torch.sin(pts[..., 0]) * 0.5 + 0.05 * pts[..., 2]
    T0 = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1).cuda()
    poses = []
    for method in ("walk", "grid"):
        p = pts.cuda()
        icp = ICP(icp_type="pt2pl", differentiable=True, max_iterations=3, tolerance=1e-12)
        icp.const_iter = True
        poses.append(icp.icp(src.cuda(), torch.cat((p, estimate_normals(p, k=12, method=method)), -1), T0, trim_dist=5.0, dim=3)["T"])
    assert torch.equal(poses[0], poses[1]) and not torch.equal(poses[0], T0)


# ------------------------------------------------------------------ 10. / 11. no host synchronisation, graph capture
def test_no_host_synchronisation():
    P = bc.random_pair(1, 5000, np.float32)[1]
    x = torch.from_numpy(P).cuda().unsqueeze(0).requires_grad_(True)
    rows = torch.tensor([4000], dtype=torch.int32).cuda()
    vp = torch.tensor(VP, dtype=torch.float32).cuda()
    estimate_normals(x, k=16, method="grid")                # (the library is loaded)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        nrm, curv, nbr = estimate_normals(x, k=16, viewpoint=vp, rows=rows, return_curvature=True, return_neighbors=True, method="grid")
        (nrm.sum() + curv.sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert np.array_equal(nbr[0, :4000].cpu().numpy(), _knn_oracle(P[:4000], 16)) and (nbr[0, 4000:] == -1).all()
    assert torch.isfinite(x.grad).all() and (x.grad[0, 4000:] == 0).all() and (x.grad[0, :4000] != 0).any()


def test_a_captured_call_replays_to_the_same_bits():
    P = bc.random_pair(1, 5000, np.float32)[1]
    xs = torch.from_numpy(P).cuda()
    eager = estimate_normals(xs, k=16, return_curvature=True, return_neighbors=True, method="grid")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        estimate_normals(xs, k=16, return_curvature=True, return_neighbors=True, method="grid")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = estimate_normals(xs, k=16, return_curvature=True, return_neighbors=True, method="grid")
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    P2 = bc.random_pair(1, 5000, np.float32, seed=1)[1]     # another cloud through the same graph: nothing of the first is baked in
    xs.copy_(torch.from_numpy(P2))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(outs[2].cpu().numpy(), _knn_oracle(P2, 16))
    assert outs[0].cpu().numpy().tobytes() == estimate_normals(torch.from_numpy(P2).cuda(), k=16).cpu().numpy().tobytes()
