"""knn_points / ball_query / chamfer_distance with deterministic=True on the MI355X.

The entry point dicp_knn_backward_y_det on designed index tensors -- lists around every edge of a chunk and of the hub threshold, hubs of
several rounds, two hubs in one wave, a hub in the last, partial workgroup, ragged row counts, a misaligned base, six columns -- against
the numpy restatement tests/knn_det_ref.py bit for bit, into a buffer that starts as NaN.  Then through the operators on the hard
layouts of tests/walk_layouts.py and on a collapsed source cloud: the forward and the x-gradient equal the default call's bit for bit,
the y-gradient equals the restatement on the returned idx bit for bit, lies within the derived bound of the exact sum, agrees with the
atomic path within the sum of both bounds, and is the same bytes under "walk" and "grid".  Then Chamfer, the input forms, cotangents in
empty slots, repeats, no host synchronisation, a captured graph, and the end-to-end chains."""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import _lib
from dicp_amd._ops import _DT, _p
from dicp_amd.ICP import ICP
from dicp_amd.ball import ball_query
from dicp_amd.fps import sample_farthest_points
from dicp_amd.group import DET_CHUNK, _invert, group_points
from dicp_amd.knn import DET_HUB, chamfer_distance, knn_points
from dicp_amd.voxel import voxel_downsample

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_ref as gr  # noqa: E402
import inverse_ref as ir  # noqa: E402
import knn_det_ref as kr  # noqa: E402
import walk_layouts as wl  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
D, H = DET_CHUNK, DET_HUB


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, misalign=False):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misalign:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _ref(g, idx, x, y, rows):
    """the restatement on one cloud, from the numpy index of idx"""
    off, slots = ir.invert_ref(idx, y.shape[0], rows)
    return kr.knn_det_ref(g, idx, x, y, rows, off, slots, fast=True)


# ------------------------------------------------------------------ 1. the entry point on designed lists
@pytest.mark.parametrize("misalign,c", [(False, 3), (True, 6)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_entry_point_on_designed_lists(dtype, misalign, c):
    """N = 3, n k = 40000 slots a cloud, m = 300 rows: 900 rows are three full workgroups and one of 132.  Cloud 0: hubs at lanes 0 and 63
    of the first wave, lists of 0, 1, D - 1, D, D + 1 and H D - 1, H D, H D + 1 entries, and a hub of 64 D + 1 entries (two rounds of
    the wave).  Cloud 1 (200 live rows): every kind of slot (inverse_ref.make_idx).  Cloud 2 (295 live rows): a hub at row 290, in the
    last workgroup, and a named row past the count."""
    N, n, k, m = 3, 5000, 8, 300
    rows = [300, 200, 295]
    deg0 = {0: H * D + 1, 63: H * D + 5, 2: 1, 3: D - 1, 4: D, 5: D + 1, 6: H * D - 1, 7: H * D, 8: H * D + 1, 100: 64 * D + 1}
    deg2 = {290: 1000, 5: 10, 299: 7}
    cases = [kr.make_case(n, k, m, rows[0], deg0, dtype, 1, cx=c, cy=c), kr.make_case(n, k, m, rows[1], {}, dtype, 2, cx=c, cy=c),
             kr.make_case(n, k, m, rows[2], deg2, dtype, 3, cx=c, cy=c)]
    cases[1]["idx"] = ir.make_idx(n, k, m, rows[1], 4, np.int64)
    cases[1]["g"] = np.where(ir.slot_rows(cases[1]["idx"], m, rows[1]) >= 0, np.nan_to_num(cases[1]["g"], nan=1.5, posinf=-2.5), np.inf).astype(dtype)
    deg = np.diff(ir.invert_ref(cases[0]["idx"], m, rows[0])[0])
    assert all(deg[j] == d for j, d in deg0.items()) and deg[1] == 0 and (N * m) % 256 != 0 and 2 * m + 290 >= (N * m) // 256 * 256
    g, idx, x, y = (np.stack([a[key] for a in cases]) for key in ("g", "idx", "x", "y"))
    gd, idd, xd, yd = _dev(g, misalign), _dev(idx), _dev(x, misalign), _dev(y, misalign)
    rd = torch.tensor(rows, dtype=torch.int32).cuda()
    off, slots = _invert(idd, rd, m)
    buf = torch.full((N * m * c + 1,), float("nan"), dtype=TORCH[dtype], device="cuda")
    gy = buf[1:].view(N, m, c) if misalign else buf[:-1].view(N, m, c)
    _lib.call("dicp_knn_backward_y_det", gd.device, _DT[gd.dtype], _p(gd), _p(idd), _p(rd), _p(xd), c, n, _p(yd), c, m, N, k, _p(off), _p(slots), _p(gy))
    got = _np(gy)
    for b in range(N):
        want = _ref(g[b], idx[b], x[b], y[b], rows[b])
        assert gr.same_bits(got[b], want), b
        assert np.isfinite(got[b]).all() and (got[b, rows[b]:] == 0).all() and (got[b, :, 3:] == 0).all()
    assert (got[0, [j for j, d in deg0.items() if d >= D - 1], :3] != 0).all() and (got[2, 290, :3] != 0).all() and (got[2, 299] == 0).all()


# ------------------------------------------------------------------ 2. through the operators
def _collapsed(n, m, seed):
    """a collapsed source: n queries within 1e-4 of one point of the unit cube, m targets in the cube -- one nearest target for all"""
    rng = np.random.default_rng(seed)
    return 0.5 + 1e-4 * rng.standard_normal((n, 3)), wl.cube(m, seed + 1)


def _layout(name, dtype):
    if name == "collapsed":
        return _collapsed(5000, 2000, 3)
    x, y, _ = wl.knn_layout(name, dtype)
    return x, y


def _run(fn, X, Y, g, **kw):
    x, y = torch.from_numpy(X).cuda().requires_grad_(True), torch.from_numpy(Y).cuda().requires_grad_(True)
    d2, idx = fn(x, y, **kw)[:2]
    torch.autograd.backward(d2, torch.from_numpy(g).cuda())
    return _np(d2), _np(idx), _np(x.grad), _np(y.grad)


def _hold(runs, X, Y, g, dtype, what, min_degree):
    """runs: {name: (default results, deterministic results)} of searches that return the same idx"""
    first = None
    for name, (a, b) in runs.items():
        assert gr.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]), (what, name)      # d2, idx: the default call's
        assert gr.same_bits(a[2], b[2]), (what, name)                                        # x.grad: the default path's
        if first is None:
            first = name
            idx = b[1]
            want = _ref(g, idx, X, Y, None)
            S, B, deg, By = kr.knn_det_bound(g, idx, X, Y, None, dtype)
            assert deg.max() >= min_degree, (what, int(deg.max()))
            r = wl.assert_within(b[3], S, B, "%s %s: deterministic y-gradient" % (what, name))
            print("%s %s: max in-degree %d, worst error / bound %.3f" % (what, np.dtype(dtype).name, deg.max(), r))
        assert np.array_equal(b[1], idx)
        assert gr.same_bits(b[3], want), (what, name)                                        # the restatement; walk and grid: the same bytes
        wl.assert_within(a[3], b[3].astype(np.longdouble), B + By, "%s %s: atomic against deterministic" % (what, name))


KNN_CASES = [("wall", 8, 1), ("cube_k16", 8, 1), ("sparse_queries", 32, 1), ("dense_queries", 8, 1000), ("dense_queries", 1, 100), ("two_clusters", 32, 1), ("edge_m+257", 1, 1),
             ("collapsed", 1, 5000), ("collapsed", 8, 5000), ("collapsed", 32, 5000)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,k,min_degree", KNN_CASES)
def test_knn_points_walk_and_grid(name, k, min_degree, dtype):
    x, y = _layout(name, dtype)
    X, Y = x.astype(dtype), y.astype(dtype)
    g = np.random.default_rng(7).standard_normal((X.shape[0], k)).astype(dtype)
    runs = {meth: tuple(_run(knn_points, X, Y, g, k=k, method=meth, deterministic=det) for det in (False, True)) for meth in ("walk", "grid")}
    _hold(runs, X, Y, g, dtype, "%s k=%d" % (name, k), min_degree)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,radius,min_degree", [("cube", 0.08, 1), ("collapsed", 0.1, 5000)])
def test_ball_query(name, radius, min_degree, dtype):
    x, y = (wl.cube(3000, 0), wl.cube(3000, 1)) if name == "cube" else _collapsed(5000, 2000, 5)
    X, Y = x.astype(dtype), y.astype(dtype)
    g = np.random.default_rng(8).standard_normal((X.shape[0], 16)).astype(dtype)
    runs = {"ball": tuple(_run(ball_query, X, Y, g, radius=radius, k=16, deterministic=det) for det in (False, True))}
    assert (runs["ball"][1][1] < 0).any() and (runs["ball"][1][1] >= 0).any()              # empty slots and live ones
    _hold(runs, X, Y, g, dtype, "ball %s" % name, min_degree)


# ------------------------------------------------------------------ 3. Chamfer
def _chamfer_case(dtype):
    rng = np.random.default_rng(11)
    N, n, m = 2, 700, 900
    X, Y = rng.random((N, n, 3)).astype(dtype), rng.random((N, m, 3)).astype(dtype)
    X[1] = (0.5 + 1e-3 * rng.standard_normal((n, 3))).astype(dtype)                       # cloud 1: a collapsed source, one hub in y
    return X, Y, [700, 650], [800, 900]


def _chamfer_grads(X, Y, xr, yr, **kw):
    x, y = torch.from_numpy(X).cuda().requires_grad_(True), torch.from_numpy(Y).cuda().requires_grad_(True)
    loss = chamfer_distance(x, y, x_rows=torch.tensor(xr), y_rows=torch.tensor(yr), reduction="sum", **kw)
    loss.backward()
    return _np(loss), _np(x.grad), _np(y.grad)


@pytest.mark.parametrize("method", ["walk", "grid"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_chamfer_both_gradients(dtype, method):
    """each cloud's gradient = the x-gradient of the search it queries in (k = 1: one term, (T)(2 g (x - y)) formed in float64) + the
    restatement of the search it is the target of, one addition in T: bit for bit"""
    X, Y, xr, yr = _chamfer_case(dtype)
    loss, gx, gy = _chamfer_grads(X, Y, xr, yr, method=method, deterministic=True)
    loss0, gx0, gy0 = _chamfer_grads(X, Y, xr, yr, method=method)
    assert gr.same_bits(loss, loss0)
    u = wl.U[np.dtype(dtype)]
    hub = 0
    for b in range(2):
        A, Bc = X[b, :xr[b]], Y[b, :yr[b]]
        want = []
        for P, Q in ((A, Bc), (Bc, A)):                     # P queries, Q targets
            _, io = wl.knn_oracle(P, Q, 1)
            g = np.full((P.shape[0], 1), dtype(1) / dtype(P.shape[0]), dtype=dtype)
            f = 2.0 * g.astype(np.float64)
            gq = (f * (P.astype(np.float64) - Q[io[:, 0]].astype(np.float64))).astype(dtype)
            want.append((gq, _ref(g, io, P, Q, None), kr.knn_det_bound(g, io, P, Q, None, dtype)))
        (gq_x, gt_y, bd_y), (gq_y, gt_x, bd_x) = want
        hub = max(hub, int(bd_y[2].max()))
        assert gr.same_bits(gx[b, :xr[b]], (gq_x + gt_x).astype(dtype)) and gr.same_bits(gy[b, :yr[b]], (gq_y + gt_y).astype(dtype)), b
        assert (gx[b, xr[b]:] == 0).all() and (gy[b, yr[b]:] == 0).all()
        for got, ref, gq, bd in ((gx0[b, :xr[b]], gx[b, :xr[b]], gq_x, bd_x), (gy0[b, :yr[b]], gy[b, :yr[b]], gq_y, bd_y)):
            # the atomic path's sum differs by at most both bounds; the final addition rounds each sum once more
            wl.assert_within(got, ref.astype(np.longdouble), (bd[1] + bd[3]) * (1 + u) + 2 * u * (np.abs(ref) + np.abs(gq) + bd[1] + bd[3]), "chamfer atomic")
    assert hub > H * D                                      # the collapsed cloud's nearest target is summed by its wave


# ------------------------------------------------------------------ 4. input forms, empty slots, repeats
def test_list_and_cpu_forms_equal_the_batch():
    X, Y, xr, yr = _chamfer_case(np.float32)
    g = np.random.default_rng(12).standard_normal((2, 700, 8)).astype(np.float32)

    def grads(x, y, gs, **kw):
        leaves = [t.requires_grad_(True) for t in (x if isinstance(x, list) else [x])] + [t.requires_grad_(True) for t in (y if isinstance(y, list) else [y])]
        d2 = knn_points(x, y, k=8, deterministic=True, **kw)[0]
        torch.autograd.backward(d2, gs)
        return d2, [t.grad for t in leaves]
    gd = torch.from_numpy(g).cuda()
    d2, (gx, gy) = grads(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), gd, x_rows=torch.tensor(xr), y_rows=torch.tensor(yr))
    assert (gy != 0).any()
    _, gl = grads([torch.from_numpy(X[b, :xr[b]]).cuda() for b in range(2)], [torch.from_numpy(Y[b, :yr[b]]).cuda() for b in range(2)], [gd[b, :xr[b]] for b in range(2)])
    for b in range(2):
        assert torch.equal(gl[b], gx[b, :xr[b]]) and torch.equal(gl[2 + b], gy[b, :yr[b]])
    dc, (cx, cy) = grads(torch.from_numpy(X.copy()), torch.from_numpy(Y.copy()), torch.from_numpy(g), x_rows=torch.tensor(xr), y_rows=torch.tensor(yr))
    assert not dc.is_cuda and not cy.is_cuda and torch.equal(dc, d2.detach().cpu()) and torch.equal(cx, gx.cpu()) and torch.equal(cy, gy.cpu())
    lo, lx, ly = _chamfer_grads(X, Y, xr, yr, deterministic=True)
    xs, ys = [torch.from_numpy(X[b, :xr[b]]).cuda().requires_grad_(True) for b in range(2)], [torch.from_numpy(Y[b, :yr[b]]).cuda().requires_grad_(True) for b in range(2)]
    chamfer_distance(xs, ys, reduction="sum", deterministic=True).backward()
    for b in range(2):
        assert gr.same_bits(_np(xs[b].grad), lx[b, :xr[b]]) and gr.same_bits(_np(ys[b].grad), ly[b, :yr[b]])


@pytest.mark.parametrize("op", ["walk", "grid", "ball"])
def test_cotangents_in_empty_slots(op):
    """m = 5 targets and k = 8 (ball_query: a radius that leaves slots empty): NaN and inf arrive at the slots with idx = -1 and y.grad is
    finite and unchanged"""
    rng = np.random.default_rng(13)
    X, Y = rng.random((300, 3)).astype(np.float32), rng.random((5 if op != "ball" else 400, 3)).astype(np.float32)
    fn = (lambda x, y, **kw: ball_query(x, y, 0.15, k=8, **kw)) if op == "ball" else (lambda x, y, **kw: knn_points(x, y, k=8, method=op, **kw))
    g = rng.standard_normal((300, 8)).astype(np.float32)
    _, idx, gx, gy = _run(fn, X, Y, g, deterministic=True)
    assert (idx < 0).any() and (idx >= 0).any()
    bad = np.where(idx < 0, np.where(rng.integers(0, 2, size=idx.shape) == 0, np.nan, np.inf), g).astype(np.float32)
    _, _, gx2, gy2 = _run(fn, X, Y, bad, deterministic=True)
    assert np.isfinite(gy2).all() and gr.same_bits(gy, gy2) and gr.same_bits(gx, gx2) and (gy != 0).any()


@pytest.mark.parametrize("hub", [False, True])
def test_runs_repeat(hub):
    """necessary, not sufficient (the restatement above is the check): three runs of every operator give equal bytes"""
    x, y = _collapsed(5000, 2000, 21) if hub else (wl.cube(5000, 21), wl.cube(2000, 22))
    X, Y = x.astype(np.float32), y.astype(np.float32)
    g = np.random.default_rng(23).standard_normal((5000, 8)).astype(np.float32)

    def once():
        out = [_run(knn_points, X, Y, g, k=8, method=meth, deterministic=True)[2:] for meth in ("walk", "grid")]
        out.append(_run(ball_query, X, Y, g, radius=0.1, k=8, deterministic=True)[2:])
        out.append(_chamfer_grads(X[None], Y[None], [5000], [2000], deterministic=True)[1:])
        return [t.tobytes() for pair in out for t in pair]
    runs = [once() for _ in range(3)]
    assert runs[1] == runs[0] and runs[2] == runs[0]


# ------------------------------------------------------------------ 5. no host synchronisation, a captured graph
def _device_case(seed):
    rng = np.random.default_rng(seed)
    X, Y = rng.random((2, 700, 3)).astype(np.float32), rng.random((2, 900, 3)).astype(np.float32)
    X[1] = (0.5 + 1e-3 * rng.standard_normal((700, 3))).astype(np.float32)
    return {"x": torch.from_numpy(X).cuda(), "y": torch.from_numpy(Y).cuda(), "g": torch.from_numpy(rng.standard_normal((2, 700, 8)).astype(np.float32)).cuda()}


def _all_ops(t, xr, yr):
    """forward + backward of the three operators and Chamfer on device tensors -> the gradients"""
    outs = []
    for fn in (lambda x, y: knn_points(x, y, k=8, x_rows=xr, y_rows=yr, deterministic=True), lambda x, y: knn_points(x, y, k=8, x_rows=xr, y_rows=yr, method="grid", deterministic=True),
               lambda x, y: ball_query(x, y, 0.2, k=8, x_rows=xr, y_rows=yr, deterministic=True)):
        x, y = t["x"].detach().requires_grad_(True), t["y"].detach().requires_grad_(True)
        outs += list(torch.autograd.grad(fn(x, y)[0], [x, y], t["g"]))
    for meth in ("walk", "grid"):
        x, y = t["x"].detach().requires_grad_(True), t["y"].detach().requires_grad_(True)
        outs += list(torch.autograd.grad(chamfer_distance(x, y, x_rows=xr, y_rows=yr, method=meth, deterministic=True), [x, y]))
    return outs


def test_no_host_synchronisation():
    t = _device_case(31)
    xr, yr = torch.tensor([700, 650], dtype=torch.int32).cuda(), torch.tensor([800, 900], dtype=torch.int32).cuda()
    _all_ops(t, xr, yr)                                     # (the library is loaded)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = _all_ops(t, xr, yr)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert all(torch.isfinite(o).all() and (o != 0).any() for o in outs)


def test_captured_forward_and_backward():
    """forward + backward (the index built inside the backward) captured once and replayed on new data in the same buffers behind
    synchronisations: the replay equals the eager call on the same data bit for bit"""
    xr, yr = torch.tensor([700, 650], dtype=torch.int32).cuda(), torch.tensor([800, 900], dtype=torch.int32).cuda()
    static = _device_case(41)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _all_ops(static, xr, yr)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = _all_ops(static, xr, yr)
    for seed in (42, 43):
        fresh = _device_case(seed)
        for key, v in fresh.items():
            static[key].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        eager = _all_ops(fresh, xr, yr)
        for i, (a, b) in enumerate(zip(cap, eager)):
            assert gr.same_bits(_np(a), _np(b)) and (a != 0).any(), (seed, i)


# ------------------------------------------------------------------ 6. the chains
def _scan(seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.random((3, 600, 3)) * 3.0).astype(np.float32)).cuda(), torch.tensor([600, 500, 430], dtype=torch.int32).cuda()


def _front_chain(scan0, rows, det, G4, cut=False):
    """voxel_downsample -> sample_farthest_points -> ball_query -> group_points(centers=) -> a loss on d2 and on the grouped tensor.
    -> scan.grad; with cut also (pts.grad, pts, idx of the ball query, the centres, the row counts) for the bound"""
    scan = scan0.clone().requires_grad_(True)
    cloud, crow = voxel_downsample(scan, 0.25, rows=rows)
    pts, _, prow = sample_farthest_points(cloud, 200, rows=crow, return_rows=True)
    if cut:
        pts.retain_grad()
    centres, _, erow = sample_farthest_points(pts, 32, rows=prow, return_rows=True)
    d2, idx = ball_query(centres, pts, 0.7, 16, x_rows=erow, y_rows=prow, deterministic=det)
    grouped = group_points(pts, idx, rows=prow, centers=centres, deterministic=det)
    loss = torch.where(idx >= 0, d2, torch.zeros_like(d2)).sum() + (grouped * G4).sum()
    loss.backward()
    if cut:
        return scan.grad, pts.grad, pts.detach(), idx, centres.detach(), prow, erow
    return scan.grad


def test_front_chain_repeats_and_the_default_agrees_within_its_bound():
    """deterministic=True: the gradient at the raw scan points is the same bytes on three runs.  deterministic=False: the same chain
    agrees with it within a bound propagated from the two scatters that differ (never asserted to differ).  At the FPS output `pts`
    the runs differ in ball_query's y-gradient -- by at most B + By (knn_det_ref.knn_det_bound: both paths' distance from the exact sum)
    -- and in group_points' feature gradient -- both orders within (deg + 2) u sum |cotangent| of the exact sum (test_gpu_group.py's
    bound; the chunked order adds at most min(deg, 64) + ceil(deg / 64) roundings) -- while the contributions through the centres are
    the same bits.  Autograd adds these contributions in one fixed order: every addition rounds once in each run, at most u times
    the sum of the magnitudes, itself at most |pts.grad| + 2 (A_ball + A_group).  Behind `pts` the backward is linear with non-negative
    weights -- FPS copies rows, voxel_downsample divides by the voxel's count, one rounding -- so the bound is sent through the same
    backward, with u |value| for each of the two runs' rounding of the division."""
    scan0, rows = _scan(51)
    G4 = torch.from_numpy(np.random.default_rng(52).standard_normal((3, 32, 16, 3)).astype(np.float32)).cuda()
    runs = [_front_chain(scan0, rows, True, G4) for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]) and (runs[0] != 0).any() and torch.isfinite(runs[0]).all()
    sg, pg, pts, idx, centres, prow, erow = _front_chain(scan0, rows, True, G4, cut=True)
    assert torch.equal(sg, runs[0])
    u = wl.U[np.dtype(np.float32)]
    Bp = np.zeros(tuple(pts.shape), dtype=np.float64)
    idn, P, Cn, G4n = _np(idx), _np(pts), _np(centres), _np(G4)
    for b in range(3):
        nb, mb = int(erow[b]), int(prow[b])
        g = (idn[b, :nb] >= 0).astype(np.float32)           # the cotangent of d2: 1 on live slots
        _, B, deg, By = kr.knn_det_bound(g, idn[b, :nb], Cn[b, :nb], P[b], mb, np.float32)
        A_ball = By / ((deg + 2) * u)[:, None]
        live = idn[b, :nb] >= 0
        A_group = np.zeros((P.shape[1], 3))
        np.add.at(A_group, idn[b, :nb][live], np.abs(G4n[b, :nb][live]).astype(np.float64))
        Bp[b] = B + By + 2 * ((deg + 2) * u)[:, None] * A_group + 4 * u * (np.abs(_np(pg)[b]) + 2 * (A_ball + A_group))
    scan2 = scan0.clone().requires_grad_(True)
    cloud2, crow2 = voxel_downsample(scan2, 0.25, rows=rows)
    pts2 = sample_farthest_points(cloud2, 200, rows=crow2)[0]
    sent, = torch.autograd.grad(pts2, scan2, torch.from_numpy(Bp).to(torch.float32).cuda() * (1 + 2.0 ** -20))
    bound = _np(sent).astype(np.float64) * (1 + 8 * u) + 4 * u * np.abs(_np(sg))
    got = _np(_front_chain(scan0, rows, False, G4))
    wl.assert_within(got, _np(sg).astype(np.longdouble), bound, "the default chain against the deterministic one")


def _icp_chain(scan0, rows, w0, det):
    src = scan0.clone().requires_grad_(True)
    w = w0.clone().requires_grad_(True)
    target = scan0 * 1.01 + 0.02
    T0 = torch.eye(4, dtype=torch.float32, device="cuda").repeat(3, 1, 1)
    icp = ICP(icp_type="pt2pt", differentiable=True, max_iterations=3, tolerance=1e-12)
    icp.deterministic = det
    out = icp.icp(src, target, T0, weight=w, source_rows=rows, target_rows=rows)
    chamfer_distance(out["pc"][..., :3], target, x_rows=rows, y_rows=rows, deterministic=det).backward()
    return src.grad, w.grad


def test_icp_chamfer_chain_repeats():
    """ICP(differentiable=True) with ICP.deterministic -> chamfer_distance(deterministic=True) -> backward: the gradients at the raw
    scan points and at `weight` are the same bytes on three runs; the default chain runs and gives finite gradients"""
    scan0, rows = _scan(61)
    w0 = torch.from_numpy((np.random.default_rng(62).random((3, 600)) + 0.5).astype(np.float32)).cuda()
    runs = [_icp_chain(scan0, rows, w0, True) for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1])
    assert (runs[0][0] != 0).any() and (runs[0][1] != 0).any() and torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()
    d = _icp_chain(scan0, rows, w0, False)
    assert torch.isfinite(d[0]).all() and torch.isfinite(d[1]).all()
