"""group_points and interpolate_features on the MI355X against their definition (dicp_amd/group.py).

The forward of every kernel form (narrow rows, wide rows with 16-byte accesses, their misaligned fallback, the scalar form of odd widths,
both dtypes, both index widths, one case beyond any grid stride) against the numpy restatement tests/group_ref.py -- bit for bit, the
interpolation within its derived bound against float64; every input form against the others bit for bit; the gradients
against an autograd graph built in torch float64 from the same indices (clamp, gather, mask), with bounds that one lost or doubled
contribution breaks; reproducibility; no host synchronisation; and the chain
voxel -> FPS -> ball -> group -> max -> knn -> interpolate -> ICP(weight=) -> backward.  Indices are made by numpy, not by the neighbour
kernels, except in the chain."""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.ICP import ICP
from dicp_amd.ball import ball_query
from dicp_amd.fps import sample_farthest_points
from dicp_amd.group import group_points, interpolate_features
from dicp_amd.knn import knn_points
from dicp_amd.voxel import voxel_downsample

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_ref as gr  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
NS, MS, KS = (1, 63, 700), (1, 257, 2000), (1, 3, 8, 32)
CS = (1, 3, 4, 6, 16, 33, 64, 65, 130)
EPS = 1e-8


def _u(dtype):
    return float(np.finfo(dtype).eps) / 2


def _table(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random(shape) * 2 - 1) * 10.0 ** rng.integers(-2, 3, size=shape)).astype(dtype)


def _dev(a, misalign=False):
    """the array on the device; misalign: as a contiguous view that starts one element into its allocation (no 16-byte base)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misalign:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _np(t):
    return t.detach().cpu().numpy()


def _batch(n, m, k, C, dtype, it, seed):
    """two clouds, the first with fewer live rows than the table holds: features, idx, d2, centres, rows"""
    rows = [m * 3 // 4, m]
    f = _table((2, m, C), dtype, seed)
    idx = np.stack([gr.make_idx(n, k, m, rows[b], seed + 10 + b, it) for b in range(2)])
    d2 = np.stack([gr.make_d2(n, k, seed + 20 + b, dtype) for b in range(2)])
    cen = _table((2, n, min(3, C)), dtype, seed + 30)
    return f, idx, d2, cen, rows


def _hold_forward(f, idx, d2, cen, rows, misalign=False):
    """every forward of one batch against the restatement, cloud by cloud"""
    dtype = f.dtype.type
    k = idx.shape[2]
    fd, idd, dd, cd = _dev(f, misalign), _dev(idx), _dev(d2), _dev(cen)
    rd = torch.tensor(rows, dtype=torch.int32).cuda()
    g0, g1 = _np(group_points(fd, idd, rows=rd)), _np(group_points(fd, idd, rows=rd, centers=cd))
    it = _np(interpolate_features(fd, idd, dd, eps=EPS, rows=rd))
    for b in range(f.shape[0]):
        assert gr.same_bits(g0[b], gr.group_ref(f[b], idx[b], rows[b]))
        assert gr.same_bits(g1[b], gr.group_ref(f[b], idx[b], rows[b], cen[b]))
        ex, sc = gr.interp_exact(f[b], idx[b], d2[b], EPS, rows[b])
        err = np.abs(it[b].astype(np.float64) - ex)
        assert (err <= gr.interp_bound(k, dtype) * sc).all(), float((err / np.maximum(gr.interp_bound(k, dtype) * sc, 1e-300)).max())


# ------------------------------------------------------------------ 1. the forward of every form
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", CS)
def test_forward_matches_reference(C, dtype):
    """every k, with n, m and the index width going round (each of n, m at every k over the C's)"""
    for a, k in enumerate(KS):
        o = a + CS.index(C)
        n, m, it = NS[o % 3], MS[(o // 3 + a) % 3], (np.int64, np.int32)[o % 2]
        _hold_forward(*_batch(n, m, k, C, dtype, it, 1000 * C + k))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_shape_at_one_width(dtype):
    """n x m in full, at the two widths where a remainder shows (narrow C = 3; wide with a tail C = 65), int32 and int64 by turns"""
    for i, n in enumerate(NS):
        for j, m in enumerate(MS):
            _hold_forward(*_batch(n, m, 8, 3, dtype, (np.int64, np.int32)[(i + j) % 2], 50 + 3 * i + j))
            _hold_forward(*_batch(n, m, 3, 65, dtype, (np.int32, np.int64)[(i + j) % 2], 70 + 3 * i + j))


@pytest.mark.parametrize("dtype", DTYPES)
def test_misaligned_base_takes_the_scalar_form(dtype):
    for C in (16, 64):
        _hold_forward(*_batch(63, 257, 8, C, dtype, np.int64, 90 + C), misalign=True)


# Every kernel is a grid-stride loop of at most 2048 workgroups: 4 queries a workgroup in the wide forms (wraps from 8192 queries on), 256
# elements a workgroup in the flat ones (wraps from 524288 elements on).  The two cases below put every kernel past its cap, forward and
# backward, and hold the results as everywhere else.
def _big_wide():
    """N = 2, n = 5000, m = 20000, C = 64, k = 16: 10000 queries = 2500 workgroups of the wide forms, 10 M elements (41 MB) of grouped output"""
    N, n, m, C, k = 2, 5000, 20000, 64, 16
    rng = np.random.default_rng(5)
    f = rng.standard_normal((N, m, C)).astype(np.float32)
    idx = rng.integers(-1, m, size=(N, n, k))
    idx[:, 17] = -1                                         # a query without a live slot in each cloud
    d2 = rng.random((N, n, k)).astype(np.float32)
    cen = rng.standard_normal((N, n, 3)).astype(np.float32)
    return f, idx, d2, cen


def test_beyond_any_grid_stride_wide_forward():
    f, idx, d2, cen = _big_wide()
    N, k = f.shape[0], idx.shape[2]
    assert N * idx.shape[1] > 2048 * 4
    fd, idd = _dev(f), _dev(idx)
    got = _np(group_points(fd, idd, centers=_dev(cen)))
    it = _np(interpolate_features(fd, idd, _dev(d2), eps=EPS))          # the batch in one call: 2500 workgroups
    for b in range(N):
        assert gr.same_bits(got[b], gr.group_ref(f[b], idx[b], None, cen[b]))
        ex, sc = gr.interp_exact(f[b], idx[b], d2[b], EPS)
        assert (np.abs(it[b].astype(np.float64) - ex) <= gr.interp_bound(k, np.float32) * sc).all()


def test_beyond_any_grid_stride_wide_backward():
    f, idx, d2, cen = _big_wide()
    _grad_case(f, idx, d2, cen, None, 700)


def test_beyond_any_grid_stride_narrow():
    """N = 2, n = 100000, m = 5000, C = 3, k = 3: 1.8 M grouped elements, 600000 (query, channel), (query, slot) and centre elements -- each
    more than 2048 x 256, so the flat forward and backward kernels of both operators and the centre-gradient kernel all wrap"""
    n, m, k, C = 100000, 5000, 3, 3
    assert 2 * n * min(C, k) > 2048 * 256
    f, idx, d2, cen, rows = _batch(n, m, k, C, np.float32, np.int64, 800)
    _hold_forward(f, idx, d2, cen, rows)
    _grad_case(f, idx, np.where(d2 == 0, np.float32(1e-3), d2), cen, rows, 801)


# ------------------------------------------------------------------ 2. input forms
@pytest.mark.parametrize("dtype", DTYPES)
def test_input_forms_agree(dtype):
    n, m, k, C = 63, 257, 8, 6
    f, idx, d2, cen, rows = _batch(n, m, k, C, dtype, np.int64, 7)
    ns = [40, n]
    for b in range(2):
        idx[b, ns[b]:] = -1                                  # (what the neighbour operators give query rows past their cloud's count)
    fd, idd, dd, cd, rd = _dev(f), _dev(idx), _dev(d2), _dev(cen), torch.tensor(rows, dtype=torch.int32).cuda()

    def run(fn):
        return (fn(lambda F, I, D, Cn, **kw: group_points(F, I, centers=Cn, **kw)), fn(lambda F, I, D, Cn, **kw: group_points(F, I, **kw)),
                fn(lambda F, I, D, Cn, **kw: interpolate_features(F, I, D, eps=EPS, **kw)))
    batch = run(lambda op: _np(op(fd, idd, dd, cd, rows=rd)))
    cpu = run(lambda op: op(torch.from_numpy(f), torch.from_numpy(idx), torch.from_numpy(d2), torch.from_numpy(cen), rows=torch.tensor(rows)))
    lists = run(lambda op: op([fd[b, :rows[b]] for b in range(2)], [idd[b, :ns[b]] for b in range(2)], [dd[b, :ns[b]] for b in range(2)],
                              [cd[b, :ns[b]] for b in range(2)]))
    for o, (bt, ct, lt) in enumerate(zip(batch, cpu, lists)):
        assert not ct.is_cuda and gr.same_bits(ct.numpy(), bt), o
        assert isinstance(lt, list) and len(lt) == 2
        for b in range(2):
            assert lt[b].is_cuda and lt[b].shape[0] == ns[b] and gr.same_bits(_np(lt[b]), bt[b, :ns[b]]), (o, b)
            if rows[b] == m:                                 # a single cloud has no rows argument: the cloud whose table is all live
                single = (group_points(fd[b], idd[b], centers=cd[b]), group_points(fd[b], idd[b]), interpolate_features(fd[b], idd[b], dd[b], eps=EPS))[o]
                assert single.shape == bt[b].shape and gr.same_bits(_np(single), bt[b]), (o, b)
        assert (bt[0, ns[0]:] == 0).all()


# ------------------------------------------------------------------ 3. gradients
def _scatter(terms, flat, rows_total):
    """sum of terms (Q, k, C) per destination row flat (Q, k) -> (rows_total, C)"""
    C = terms.shape[-1]
    return torch.zeros((rows_total, C), dtype=torch.float64, device="cuda").index_add_(0, flat.reshape(-1), terms.reshape(-1, C))


def _hold_gf(got, terms, live, idx, N, m, k, u, auto):
    """g_features against the float64 sum of its terms (Q, k, C): within (D + k + 8) u sum|terms| per element, D the row's in-degree; rows
    nobody points at exactly 0.  auto: the same gradient through autograd, a check of the bookkeeping"""
    Q = terms.shape[0]
    base = (torch.arange(Q, device="cuda") // (Q // N) * m)[:, None]
    flat = idx.reshape(Q, k).clamp(min=0, max=m - 1) + base
    t = torch.where(live.reshape(Q, k, 1), terms, torch.zeros_like(terms))
    ref, ab = _scatter(t, flat, N * m), _scatter(t.abs(), flat, N * m)
    deg = torch.zeros(N * m, dtype=torch.float64, device="cuda").index_add_(0, flat.reshape(-1), live.reshape(-1).double())[:, None]
    assert torch.allclose(auto.reshape(N * m, -1), ref, rtol=1e-11, atol=1e-13)
    got = got.reshape(N * m, -1).double()
    assert torch.isfinite(got).all()
    assert (got[(deg == 0).expand_as(got)] == 0).all()
    bound = (deg + k + 8) * u * ab
    assert ((got - ref).abs() <= bound).all(), float(((got - ref).abs() - bound).max())
    return deg


def _live(idx, rows, m):
    lim = rows.view(-1, 1, 1) if rows is not None else m
    return (idx >= 0) & (idx < lim)


def _grad_case(f, idx, d2, cen, rows, seed, nan_at_empty=False):
    """the gradients of both operators on one batch (N, ...) against torch float64"""
    dtype = f.dtype.type
    tdt, u = TORCH[dtype], _u(dtype)
    N, m, C = f.shape
    n, k = idx.shape[1:]
    Q = N * n
    gen = torch.Generator().manual_seed(seed)

    def cot(shape):
        return ((torch.rand(shape, generator=gen, dtype=torch.float64) + 0.5) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).to(tdt).cuda()
    idd = _dev(idx)
    rd = torch.tensor(rows, dtype=torch.int32).cuda() if rows is not None else None
    live = _live(idd, rd, m)
    any_live = live.any(2)
    assert live.any() and (~live).any() and (~any_live).any()
    safe = idd.clamp(min=0, max=m - 1).long()
    f64 = _dev(f).double()
    bi = torch.arange(N, device="cuda")[:, None, None]
    nan = float("nan")

    # group_points
    fd, cd = _dev(f).requires_grad_(True), _dev(cen).requires_grad_(True)
    g = cot((N, n, k, C))
    out = group_points(fd, idd, rows=rd, centers=cd)
    out.backward(torch.where(live[..., None], g, torch.full_like(g, nan)) if nan_at_empty else g)
    fa, ca = f64.clone().requires_grad_(True), _dev(cen).double().requires_grad_(True)
    Cc = cen.shape[2]
    ga = fa[bi, safe] - torch.cat([ca, torch.zeros((N, n, C - Cc), dtype=torch.float64, device="cuda")], 2)[:, :, None, :]
    (torch.where(live[..., None], ga, torch.zeros_like(ga)) * g.double()).sum().backward()
    _hold_gf(fd.grad, g.double().reshape(Q, k, C), live, idd, N, m, k, u, fa.grad)
    # g_centers: -(the sum of at most k cotangents, k - 1 additions in slot order): within k u sum|g|
    gl = torch.where(live[..., None], g.double(), torch.zeros((), dtype=torch.float64, device="cuda"))[..., :Cc]
    assert torch.allclose(ca.grad, -gl.sum(2), rtol=1e-11, atol=1e-13)
    assert ((cd.grad.double() + gl.sum(2)).abs() <= k * u * gl.abs().sum(2)).all()
    assert (cd.grad[~any_live] == 0).all()

    # interpolate_features
    fd, dd = _dev(f).requires_grad_(True), _dev(d2).requires_grad_(True)
    g = cot((N, n, C))
    out = interpolate_features(fd, idd, dd, eps=EPS, rows=rd)
    out.backward(torch.where(any_live[..., None], g, torch.full_like(g, nan)) if nan_at_empty else g)
    li = live & torch.isfinite(dd.detach())
    fa = f64.clone().requires_grad_(True)
    da = torch.where(li, dd.detach().double(), torch.zeros((), dtype=torch.float64, device="cuda")).requires_grad_(True)
    r = torch.where(li, 1.0 / (da + float(dtype(EPS))), torch.zeros_like(da))
    R = r.sum(2, keepdim=True)
    w = r / torch.where(R > 0, R, torch.ones_like(R))
    gz = torch.where(li.any(2)[..., None], g.double(), torch.zeros((), dtype=torch.float64, device="cuda"))
    ((w[..., None] * fa[bi, safe]).sum(2) * gz).sum().backward()
    _hold_gf(fd.grad, (w.detach()[..., None] * gz[:, :, None, :]).reshape(Q, k, C), li, idd, N, m, k, u, fa.grad)
    gd = _np(dd.grad)
    gnp = _np(gz).astype(dtype)
    for b in range(N):
        ex, sc = gr.gd2_exact(f[b], idx[b], d2[b], EPS, gnp[b], None if rows is None else rows[b])
        assert np.allclose(_np(da.grad)[b], ex, rtol=1e-9, atol=1e-12 * max(sc.max(), 1e-300))
        err = np.abs(gd[b].astype(np.float64) - ex)
        assert (err <= gr.gd2_bound(k, C, dtype) * sc).all(), float((err / np.maximum(gr.gd2_bound(k, C, dtype) * sc, 1e-300)).max())
        assert (gd[b][~_np(li[b])] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,k,C,it", [(700, 257, 8, 3, np.int64), (63, 2000, 3, 1, np.int32), (700, 2000, 32, 33, np.int32), (63, 257, 8, 64, np.int64),
                                        (63, 257, 3, 130, np.int64), (1, 1, 1, 16, np.int64)])
def test_gradients(n, m, k, C, it, dtype):
    f, idx, d2, cen, rows = _batch(n, m, k, C, dtype, it, 400 + C)
    if n == 1:                                              # one query per cloud: a live one and an empty one
        idx[0, 0, 0], idx[1, 0, 0], rows = 0, -1, [1, 1]
    d2 = np.where(d2 == 0, dtype(1e-3), d2)                 # (torch's graph differentiates through an exact zero too: kept for the forward tests)
    _grad_case(f, idx, d2, cen, rows, 500 + C, nan_at_empty=(C % 2 == 1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [3, 64])
def test_gradient_of_one_row_everybody_points_at(C, dtype):
    """700 x 8 slots on row 5 of 257 (in-degree 5600) and one query without a live slot; every other row's gradient is exactly 0"""
    n, m, k = 701, 257, 8
    idx = np.full((1, n, k), 5, dtype=np.int64)
    idx[0, 700] = -1
    f, d2, cen = _table((1, m, C), dtype, 1), gr.make_d2(n, k, 2, dtype, near=True)[None], _table((1, n, 3), dtype, 3)
    _grad_case(f, idx, d2, cen, None, 600 + C, nan_at_empty=True)


# ------------------------------------------------------------------ 4. reproducibility, no host synchronisation
def test_runs_repeat():
    f, idx, d2, cen, rows = _batch(700, 2000, 8, 64, np.float32, np.int64, 11)
    runs = []
    for _ in range(2):
        fd, idd, dd, cd, rd = _dev(f), _dev(idx), _dev(d2).requires_grad_(True), _dev(cen).requires_grad_(True), torch.tensor(rows, dtype=torch.int32).cuda()
        a = group_points(fd, idd, rows=rd, centers=cd)
        a.backward(torch.ones_like(a) * 0.37)
        i = interpolate_features(fd, idd, dd, eps=EPS, rows=rd)
        i.backward(torch.ones_like(i) * 0.61)
        runs.append([_np(t).tobytes() for t in [a, i, cd.grad, dd.grad]])
    assert runs[0] == runs[1]


def test_no_host_synchronisation():
    f, idx, d2, cen, rows = _batch(700, 2000, 8, 64, np.float32, np.int64, 12)
    fd, idd, dd, cd, rd = _dev(f).requires_grad_(True), _dev(idx), _dev(d2).requires_grad_(True), _dev(cen).requires_grad_(True), torch.tensor(rows, dtype=torch.int32).cuda()
    group_points(fd, idd, rows=rd)                          # (the library is loaded)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = group_points(fd, idd, rows=rd, centers=cd)
        i = interpolate_features(fd, idd, dd, eps=EPS, rows=rd)
        (a.sum() + i.sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for b in range(2):
        assert gr.same_bits(_np(a[b]), gr.group_ref(f[b], idx[b], rows[b], cen[b]))
    assert torch.isfinite(fd.grad).all() and (fd.grad != 0).any() and (dd.grad != 0).any()


# ------------------------------------------------------------------ 5. the chain
def test_chain_to_icp_weights():
    rng = np.random.default_rng(21)
    scan = torch.from_numpy((rng.random((2, 3000, 3)) * 4.0).astype(np.float32)).cuda()
    target = scan + 0.02
    rows = torch.tensor([3000, 2400], dtype=torch.int32).cuda()
    cloud, crow = voxel_downsample(scan, 0.3, rows=rows)
    pts, _, prow = sample_farthest_points(cloud, 500, rows=crow, return_rows=True)                 # the two clouds of about 500 points
    centres, _, erow = sample_farthest_points(pts, 64, rows=prow, return_rows=True)
    d2, idx = ball_query(centres, pts, 0.6, 16, x_rows=erow, y_rows=prow)
    grouped = group_points(pts, idx, rows=prow, centers=centres)                                   # (2, 64, 16, 3), relative to the centre
    assert grouped.shape == (2, 64, 16, 3)
    lin = torch.linspace(-1.0, 1.0, 3, device="cuda").requires_grad_(True)                          # the user's "MLP": one linear map
    feat = (grouped * lin).sum(-1, keepdim=True)
    centre_w = torch.sigmoid(torch.where(idx >= 0, feat[..., 0], torch.full_like(feat[..., 0], -1e30)).amax(2, keepdim=True))   # max over k
    centre_w.retain_grad()
    d3, i3 = knn_points(pts, centres, k=3, x_rows=prow, y_rows=erow)
    w = interpolate_features(centre_w, i3, d3, eps=EPS, rows=erow)                                 # (2, 500, 1)
    assert w.shape == (2, 500, 1)
    T0 = torch.eye(4, dtype=torch.float32, device="cuda").repeat(2, 1, 1)
    icp = ICP(icp_type="pt2pt", differentiable=True, max_iterations=3, tolerance=1e-12)
    out = icp.icp(pts.detach(), target, T0, weight=w[..., 0], source_rows=prow, target_rows=rows)
    out["T"].sum().backward()
    gw = centre_w.grad
    assert torch.isfinite(gw).all() and (gw != 0).any() and torch.isfinite(lin.grad).all() and (lin.grad != 0).any()
    cw, i3n, d3n, wn = _np(centre_w), _np(i3), _np(d3), _np(w)
    for b in range(2):
        ex, sc = gr.interp_exact(cw[b], i3n[b], d3n[b], EPS, int(erow[b]))
        assert (np.abs(wn[b].astype(np.float64) - ex) <= gr.interp_bound(3, np.float32) * sc).all()
        assert (wn[b, :int(prow[b])] > 0).all()
