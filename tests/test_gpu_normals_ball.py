"""estimate_normals_ball on the MI355X (dicp_amd/normals.py; csrc/normals_ball.hip) against the numpy restatement
tests/normals_ball_ref.py: normals, curvature, eigenvalues and counts bit for bit, and the gradient -- the gather bit for bit on the
kernel's own records, the whole gradient against a float64 torch composition and torch.autograd.gradcheck --, float32 and float64.

1  tile and wave edges: m in {1, 2, 63, 64, 65, 300}, two clouds of different row counts per call, dead rows and extra columns holding
   NaN, c in {3, 6}, balls of about 4, 40 and 150 rows, a viewpoint per cloud;
2  eigenvalues and counts equal iss_saliency_ball's at the same radius (inside every check of 1, and on the layouts of the coverage claim);
3  the gradient: records hook, composition, gradcheck on the wavy sheet;
4  three runs give the same bytes; rows below min_neighbors CONTRIBUTE exactly nothing (their records are zero, asserted in every check;
   where no row reaches min_neighbors the whole gradient is zero), dead rows and columns >= 3 have exactly zero gradient; zero cotangents.
   A live row below min_neighbors still RECEIVES the terms of the members whose balls hold it -- rule 6 of the header, and what the
   float64 composition gives (test_gradient_against_the_composition runs the sheet with min_neighbors = 5, counts 3 .. 16);
5  the cross-check with estimate_normals(k=12, method="grid") on the cluster lattice, no row excluded;
6  single clouds, lists and CPU tensors against the batch, both viewpoint forms, a captured forward + backward, the visit counters.

Where a grid's plan enlarged an edge or went flat, the reference takes the edges from the library's own plan
(tests/test_gpu_iss_ball.py's device_plans).
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import iss as iss_module
from dicp_amd.iss import iss_saliency_ball
from dicp_amd.normals import estimate_normals, estimate_normals_ball

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iss_ball_cases as ibc  # noqa: E402
import iss_ref as ir  # noqa: E402
import normals_ball_cases as nbc  # noqa: E402
import normals_ball_ref as nbr  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
ATOL, RTOL = 1e-6, 1e-4                                     # the project's gradcheck tolerances


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def device_plans(Pd, rows_t, radius):
    """the plans of the grid the front end builds for this batch and radius -> [None where the simple rule stands, else (edges (3,),
    enlarged, flat)] per cloud (csrc/dicp_ball.h: BallPlan -- o[3], s[3], R, r2 of T, then hi[3] int64, wy, wz, cnt, flat int32)"""
    grid = iss_module._ball_grid(Pd, rows_t, radius)
    raw = host(grid.plans)
    dt = host(Pd).dtype
    ts = dt.itemsize
    out = []
    for b in range(raw.shape[0]):
        f = raw[b, :8 * ts].copy().view(dt)
        ints = raw[b, 8 * ts + 24:8 * ts + 40].copy().view(np.int32)
        edges, R, flat = f[3:6], f[6], bool(ints[3])
        enlarged = flat or bool((edges != R).any())
        out.append((edges, enlarged, flat) if enlarged else None)
    return out


def padded(clouds, cols):
    """clouds [(points (m_b, 3), rows_b)] -> P (N, m, cols) with NaN in dead rows, pad rows and extra columns, rows (N,)"""
    m = max(c[0].shape[0] for c in clouds)
    P = np.full((len(clouds), m, cols), np.nan, dtype=clouds[0][0].dtype)
    for b, (pts, r) in enumerate(clouds):
        P[b, :r, :3] = pts[:r, :3]
    return P, np.array([c[1] for c in clouds], dtype=np.int32)


def cotangents(seed, shape, dtype):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape + (3,)).astype(dtype), rng.standard_normal(shape).astype(dtype)


def check(P, rows, radius, viewpoint=None, min_neighbors=3, seed=0):
    """One batch: the forward against the reference bit for bit, eigenvalues and counts against iss_saliency_ball's, and the gather
    against the reference ON THE KERNEL'S OWN RECORDS bit for bit -> (reference, gradient (N, m, c), records by row (N, m, 13))"""
    N, m, c = P.shape
    rows_t = None if rows is None else torch.tensor(np.asarray(rows), dtype=torch.int32).cuda()
    vp_t = None if viewpoint is None else torch.from_numpy(np.asarray(viewpoint, dtype=P.dtype))
    Pd = dev(P).requires_grad_(True)
    plans = device_plans(Pd.detach(), rows_t, radius)
    ref = nbr.forward_ref_batch(P, radius, rows, viewpoint, plans=plans, min_neighbors=min_neighbors)
    records = []
    nrm, curv, eig, cnt = estimate_normals_ball(Pd, radius, viewpoint=vp_t, rows=rows_t, min_neighbors=min_neighbors, return_curvature=True,
                                                return_eigenvalues=True, return_counts=True, _records=records)
    assert nrm.shape == (N, m, 3) and curv.shape == (N, m) and eig.shape == (N, m, 3) and cnt.shape == (N, m)
    assert nrm.dtype == Pd.dtype and curv.dtype == Pd.dtype and eig.dtype == Pd.dtype and cnt.dtype == torch.int32
    assert nrm.requires_grad and curv.requires_grad and not eig.requires_grad and not cnt.requires_grad
    for key, got in (("count", cnt), ("eig", eig), ("normals", nrm), ("curv", curv)):
        assert ir.same_bits(host(got), ref[key]), key
    _, eig_i, cnt_i = iss_saliency_ball(Pd.detach(), radius, rows=rows_t, return_eigenvalues=True, return_counts=True)
    assert ir.same_bits(host(eig), host(eig_i)) and ir.same_bits(host(cnt), host(cnt_i))
    gn, gk = cotangents(seed, (N, m), P.dtype)
    grad, = torch.autograd.grad([nrm, curv], [Pd], [dev(gn), dev(gk)])
    grad = host(grad)
    assert grad.shape == P.shape and grad.dtype == P.dtype and len(records) == 1
    rec, grid = records[0]
    assert rec.shape == (N, grid.slots, nbr.REC) and rec.dtype == torch.float64
    rec, perm = host(rec), host(grid.perm)
    by_row = np.stack([nbr.records_by_row(rec[b], perm[b], m) for b in range(N)])
    on = (ref["count"] >= min_neighbors)
    assert not by_row[~on][:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 12]].any()
    live = ref["count"] > 0
    assert ir.same_bits(by_row[live][:, 9:12], P[live][:, :3].astype(np.float64))
    for b in range(N):
        want = nbr.gather_ref(P[b], by_row[b], radius, None if rows is None else int(rows[b]), plans[b])
        assert ir.same_bits(grad[b, :, :3], want), b
    assert not grad[..., 3:].any() and not grad[~live].any()
    return ref, grad, by_row


# ------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 300])
def test_tile_edges(dtype, m):
    for q, members in enumerate((4, 40, 150)):
        a, b = ibc.cube(100 * m + q, m, dtype), ibc.cube(100 * m + q + 50, m, dtype)
        if m >= 63:
            a[3, 1], a[9, 0], a[11] = np.nan, np.inf, a[10]                        # dead rows inside the cloud, an exact duplicate
        P, rows = padded([(a, m), (b, m - m // 3)], 3 if q % 2 == 0 else 6)
        radius = ibc.ball_radius(a, members) if m > 2 else 0.8
        vp = None if q == 0 else ([0.3, -2.0, 5.0] if q == 1 else [[0.3, -2.0, 5.0], [-4.0, 0.1, 0.2]])
        ref, grad, rec = check(P, rows, radius, vp, min_neighbors=3 if q else 5, seed=m + q)
        live = ref["count"][0] > 0
        if m == 300:
            assert abs(np.median(ref["count"][0][live]) - 1 - members) <= 0.5 * members      # (the ball holds what the case says)
            assert (members <= 31) == (ref["count"].max() <= 32)                             # 40 and 150: beyond the k-slot form
            assert rec[..., 12].astype(bool).sum() > 100 and np.abs(grad).max() > 0
        if m >= 63:
            assert not ref["count"][0, 3] and not ref["count"][0, 9] and not ref["count"][1, m - m // 3:].any()
            assert ir.same_bits(ref["eig"][0, 10], ref["eig"][0, 11])
        if m <= 2:
            assert not ref["normals"].any() and not grad.any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["lattice r=1.000", "radius rounds down", "two clusters", "far outlier", "flat"])
def test_layouts(dtype, name):
    """rows exactly at R, a radius whose float32 conversion rounds down, enlarged edges, a flat grid: the reference takes the library's plan"""
    pts, r, _ = ibc.layouts(dtype)[name]
    plans = device_plans(dev(pts[None]), None, r)
    assert (plans[0] is not None) == (name in ("two clusters", "far outlier", "flat")) and (plans[0] is None or plans[0][2] == (name == "flat"))
    check(pts[None], None, r, [0.5, 0.25, 40.0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["planar", "collinear", "only_itself", "non_finite"])
def test_designed_clouds(dtype, name):
    pts, rows, r, _ = ibc.designed(dtype)[name]
    P, rw = padded([(pts, rows), (ibc.cube(9, 12, dtype), 0)], 3)                  # with a cloud that has no rows
    ref, grad, rec = check(P, rw, r, [0.0, 0.0, 10.0])
    assert not ref["count"][1].any() and not ref["normals"][1].any() and not grad[1].any()
    if name == "planar":
        assert (ref["eig"][0, :8, 0] == 0).all() and (np.abs(ref["normals"][0, :8, 2]) == 1).all() and not ref["curv"].any()
    if name in ("collinear", "only_itself"):
        assert not rec[..., 12].any() and not grad.any()                           # lam_0 = lam_1; alone: no gradient


# ------------------------------------------------------------------ 3
def composition_gradient(P, radius, rows, viewpoint, min_neighbors, gn, gk):
    x = torch.from_numpy(np.where(np.isfinite(P[:, :3]), P[:, :3], 0.0).astype(np.float64)).requires_grad_(True)
    out = nbr.composition(x, radius, rows, viewpoint, min_neighbors, points=P)
    loss = (out["normals"] * torch.from_numpy(gn.astype(np.float64))).sum() + (out["curv"] * torch.from_numpy(gk.astype(np.float64))).sum()
    loss.backward()
    return x.grad.numpy()


def composition_cases(dtype):
    """[(P (N, m, c), rows, radius, viewpoint, min_neighbors)]: two cubes with dead rows at 14 members a ball and a viewpoint per cloud; the
    wavy sheet beside a cube with min_neighbors = 5"""
    a, b = ibc.cube(21, 300, dtype), ibc.cube(23, 300, dtype)
    a[3, 1], a[9, 0], a[11] = np.nan, np.inf, a[10]
    cubes = padded([(a, 300), (b, 211)], 4)
    sheet = padded([(nbc.sheet().astype(dtype), 40), (ibc.cube(24, 40, dtype), 33)], 3)
    return [cubes + (ibc.ball_radius(a, 14), [[0.5, 0.5, 3.0], [0.0, -4.0, 0.5]], 3), sheet + (nbc.SHEET_RADIUS, None, 5)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradient_against_the_composition(dtype):
    """the whole gradient against torch autograd on the CPU in float64 (constant membership mask, masked mean and covariance,
    torch.linalg.eigh, the reference's sign); for float32 points the composition runs on the points converted to double.  Asserted on
    the reference first: every row that takes part has a relative eigen gap above 1e-3, far from the tau cut of either dtype"""
    for P, rows, radius, vp, min_nb in composition_cases(dtype):
        ref, grad, rec = check(P, rows, radius, vp, min_nb, seed=5)
        gn, gk = cotangents(5, P.shape[:2], dtype)
        for c in range(P.shape[0]):
            one = nbr.forward_ref(P[c], radius, int(rows[c]), None if vp is None else vp[c], min_nb)
            lam = one["lam"][one["count"] >= min_nb]
            assert lam.shape[0] >= 20 and ((lam[:, 1] - lam[:, 0]) / lam.sum(1)).min() > 1e-3
            assert np.array_equal(rec[c][:, 12] != 0, one["count"] >= min_nb)
            want = composition_gradient(P[c], radius, int(rows[c]), None if vp is None else vp[c], min_nb, gn[c], gk[c])
            assert np.abs(want).max() > 1e-2
            assert np.allclose(grad[c, :, :3].astype(np.float64), want, rtol=RTOL, atol=ATOL), (radius, c)


def test_gradcheck_float64():
    """the wavy sheet at R = 0.7, normals and curvature together.  Asserted on the reference first: every count is 3 .. 16, the smallest
    relative eigen gap is above 0.02 and no pair is nearer than 1.5e-3 to the ball's border -- finite differences of 1e-6 cannot move a
    member and no row is at the tau cut"""
    count_min, count_max, gap, border = nbc.sheet_conditions()
    assert count_min >= 3 and count_max <= 16 and gap >= 0.02 and border >= 1.5e-3
    x = dev(nbc.sheet()).requires_grad_(True)
    f = lambda t: estimate_normals_ball(t, nbc.SHEET_RADIUS, viewpoint=torch.tensor([0.5, 0.5, 3.0], dtype=torch.float64), return_curvature=True)   # noqa: E731
    assert torch.autograd.gradcheck(f, (x,), eps=1e-6, atol=1e-6, rtol=1e-4)


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("dtype", DTYPES)
def test_reproducible_and_exact_zeros(dtype):
    a, b = ibc.cube(31, 300, dtype), ibc.cube(32, 300, dtype)
    a[3, 1], a[9, 0] = np.nan, np.inf
    P, rows = padded([(a, 300), (b, 211)], 6)
    radius, min_nb = ibc.ball_radius(a, 8), 6
    rows_t = torch.tensor(rows).cuda()
    gn, gk = (dev(t) for t in cotangents(3, (2, 300), dtype))

    def run(g_n, g_k):
        x = dev(P).requires_grad_(True)
        nrm, curv, cnt = estimate_normals_ball(x, radius, rows=rows_t, min_neighbors=min_nb, return_curvature=True, return_counts=True)
        grad, = torch.autograd.grad([nrm, curv], [x], [g_n, g_k])
        return host(nrm), host(curv), host(cnt), host(grad)
    first = run(gn, gk)
    for _ in range(2):
        assert all(ir.same_bits(u, v) for u, v in zip(run(gn, gk), first))
    nrm, curv, cnt, grad = first
    low = (cnt > 0) & (cnt < min_nb)
    assert low.sum() > 10 and (cnt >= min_nb).sum() > 100 and not nrm[low].any() and not curv[low].any()
    # a row below min_neighbors still RECEIVES gradient from the members whose ball holds it; a cloud of such rows alone gets none
    assert not grad[cnt == 0].any() and not grad[..., 3:].any() and np.abs(grad[..., :3]).max() > 0 and np.isfinite(grad).all()
    x = dev(P).requires_grad_(True)
    nrm_s = estimate_normals_ball(x, radius, rows=rows_t, min_neighbors=400)       # no row has 400 members: nothing contributes
    g_s, = torch.autograd.grad([nrm_s], [x], [gn])
    assert not host(nrm_s).any() and not host(g_s).any()
    zero = run(torch.zeros_like(gn), torch.zeros_like(gk))[3]
    assert not zero.any() and not np.signbit(zero).any()
    only_n = run(gn, torch.zeros_like(gk))[3]
    x = dev(P).requires_grad_(True)
    g_n, = torch.autograd.grad([estimate_normals_ball(x, radius, rows=rows_t, min_neighbors=min_nb)], [x], [gn])       # the curvature's cotangent absent
    assert ir.same_bits(host(g_n), only_n)


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 1e-4)])
def test_cross_check_with_the_k_slot_form(dtype, tol):
    """On the cluster lattice every ball of radius 2 holds exactly its cluster of 12 rows (asserted on the references), so
    estimate_normals(k=12) sees the SAME member sets and only the order of summation differs: the sine of the angle between the two
    normals stays within the bound tests/test_gpu_normals.py uses for rows whose relative gap is above 1e-3, here with NO row excluded
    (the smallest gap is above 0.1), and the curvature within that file's tolerances"""
    for seed in nbc.CLUSTER_SEEDS:
        own, count_min, count_max, gap, border = nbc.cluster_conditions(seed, dtype)
        assert own and count_min == count_max == 12 and gap >= 0.1 and border >= 0.5
    P = np.stack([nbc.clusters(seed, dtype) for seed in nbc.CLUSTER_SEEDS])
    Pd = dev(P)
    vp = torch.tensor([8.0, 8.0, 50.0], dtype=Pd.dtype)
    nb, cb, cnt = estimate_normals_ball(Pd, nbc.CLUSTER_RADIUS, viewpoint=vp, return_curvature=True, return_counts=True)
    nk, ck = estimate_normals(Pd, k=12, viewpoint=vp, return_curvature=True, method="grid")
    assert bool((cnt == 12).all())
    nb, nk = host(nb).astype(np.float64), host(nk).astype(np.float64)
    sine = np.linalg.norm(np.cross(nb, nk), axis=-1) / np.linalg.norm(nb, axis=-1)
    print("%s: sine of the angle max %.3g" % (np.dtype(dtype).name, sine.max()))
    assert sine.max() <= tol and (np.einsum("bma,bma->bm", nb, nk) > 0).all()
    np.testing.assert_allclose(host(cb), host(ck), rtol=1e-4 if dtype == np.float32 else 1e-9, atol=1e-6 if dtype == np.float32 else 1e-13)


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("dtype", DTYPES)
def test_forms(dtype):
    rows = [90, 61, 75]
    P, rw = padded([(ibc.cube(51 + b, 90, dtype), r) for b, r in enumerate(rows)], 4)
    P = np.where(np.isnan(P), 0.0, P).astype(dtype)                                # (finite everywhere: the list form keeps the extra column)
    radius = 0.5
    vps = np.array([[0.3, -2.0, 5.0], [-4.0, 0.1, 0.2], [0.0, 0.0, -3.0]], dtype=dtype)
    ref = nbr.forward_ref_batch(P, radius, rw, vps)
    keys = ("normals", "curv", "eig", "count")
    flags = dict(return_curvature=True, return_eigenvalues=True, return_counts=True)
    got = estimate_normals_ball(dev(P), radius, viewpoint=torch.from_numpy(vps), rows=torch.tensor(rw).cuda(), **flags)
    assert all(ir.same_bits(host(g), ref[k]) for g, k in zip(got, keys)) and ref["count"].max() > 12
    one = nbr.forward_ref_batch(P, radius, rw, vps[0])                             # one viewpoint (3,) for every cloud
    got = estimate_normals_ball(dev(P), radius, viewpoint=torch.from_numpy(vps[0]), rows=torch.tensor(rw).cuda(), **flags)
    assert all(ir.same_bits(host(g), one[k]) for g, k in zip(got, keys)) and not ir.same_bits(one["normals"], ref["normals"])
    for b, r in enumerate(rows):                                                    # single clouds
        got = estimate_normals_ball(dev(P[b, :r]), radius, viewpoint=torch.from_numpy(vps[b]), **flags)
        assert got[0].shape == (r, 3) and got[1].shape == (r,) and got[2].shape == (r, 3) and got[3].shape == (r,)
        assert all(ir.same_bits(host(g), ref[k][b, :r]) for g, k in zip(got, keys))
    got = estimate_normals_ball(dev(P[0, :90]), radius, rows=torch.tensor([50]), return_counts=True)       # a single cloud with a row count
    assert ir.same_bits(host(got[1]), nbr.forward_ref(P[0, :90], radius, 50)["count"])
    lists = estimate_normals_ball([dev(P[b, :r]) for b, r in enumerate(rows)], radius, viewpoint=torch.from_numpy(vps), **flags)
    assert all(isinstance(o, list) and len(o) == 3 for o in lists)
    assert all(ir.same_bits(host(lists[i][b]), ref[k][b, :r]) for i, k in enumerate(keys) for b, r in enumerate(rows))
    cpu = estimate_normals_ball(torch.from_numpy(P), radius, viewpoint=torch.from_numpy(vps), rows=torch.tensor(rw), **flags)
    assert all(not o.is_cuda and ir.same_bits(o.numpy(), ref[k]) for o, k in zip(cpu, keys))
    alone = estimate_normals_ball(dev(P), radius, rows=torch.tensor(rw).cuda())   # no flag: the normals alone
    assert torch.is_tensor(alone) and alone.shape == (3, 90, 3)
    # gradients through the forms: a CPU leaf gets a CPU gradient equal to the device call's
    gn = cotangents(8, (3, 90), dtype)[0]
    xd = dev(P).requires_grad_(True)
    gd, = torch.autograd.grad([estimate_normals_ball(xd, radius, rows=torch.tensor(rw).cuda())], [xd], [dev(gn)])
    xc = torch.from_numpy(P.copy()).requires_grad_(True)
    gc, = torch.autograd.grad([estimate_normals_ball(xc, radius, rows=torch.tensor(rw))], [xc], [torch.from_numpy(gn)])
    assert not gc.is_cuda and ir.same_bits(gc.numpy(), host(gd)) and np.abs(host(gd)).max() > 0


def _case(seed):
    rows = [400, 333]
    P, _ = padded([(ibc.cube(seed + b, 400, np.float32), r) for b, r in enumerate(rows)], 3)
    gn, gk = cotangents(seed, (2, 400), np.float32)
    return {"P": dev(P), "gn": dev(gn), "gk": dev(gk)}


def _forward_backward(t, rows_t, visited=None):
    x = t["P"].detach().requires_grad_(True)
    nrm, curv, eig, cnt = estimate_normals_ball(x, 0.4, rows=rows_t, return_curvature=True, return_eigenvalues=True, return_counts=True, _visited=visited)
    grad, = torch.autograd.grad([nrm, curv], [x], [t["gn"], t["gk"]])
    return nrm.detach(), curv.detach(), eig, cnt, grad


def test_captured_forward_and_backward():
    """forward + backward captured once and replayed twice on new data in the same buffers: each replay equals the eager call bit for bit"""
    rows_t = torch.tensor([400, 333], dtype=torch.int32).cuda()
    static = _case(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _forward_backward(static, rows_t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _forward_backward(static, rows_t)
    for seed in (20, 30):
        fresh = _case(seed)
        for key, t in fresh.items():
            static[key].copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = _forward_backward(fresh, rows_t)
        torch.cuda.synchronize()
        assert all(ir.same_bits(host(c), host(e)) for c, e in zip(captured, eager))
        assert int(captured[3].max()) > 32 and bool((captured[4] != 0).any())


def test_no_host_synchronisation_and_visit_counters():
    """nothing is read back; the backward visits exactly what ONE forward walk visits, the forward twice that"""
    rows_t = torch.tensor([400, 333], dtype=torch.int32).cuda()
    t = _case(7)
    _forward_backward(t, rows_t)                            # (the library is loaded)
    visited = (torch.zeros(2, dtype=torch.int64).cuda(), torch.zeros(2, dtype=torch.int64).cuda())
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with_counters = _forward_backward(t, rows_t, visited)
        without = _forward_backward(t, rows_t)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert all(ir.same_bits(host(u), host(v)) for u, v in zip(with_counters, without))          # the counters touch no output
    fwd, bwd = host(visited[0]), host(visited[1])
    assert (bwd > 0).all() and np.array_equal(fwd, 2 * bwd)
    members = host(with_counters[3]).astype(np.int64).sum(axis=1)
    assert (bwd >= members).all()                           # a walk visits every member, the row itself included
