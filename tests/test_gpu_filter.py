"""select_rows, radius_outlier_removal and statistical_outlier_removal on the MI355X against their definitions (dicp_amd/filter.py), bit
for bit against tests/filter_ref.py: the compaction with its index and gradient at every tile boundary, column count and kind of mask; the
statistical filter on the d2 / idx that knn_points returns for the same input; the radius filter on tests/ball_ref.py's counts; every input
form; no host synchronisation in the batch forms; and the chain voxel -> filter -> normals -> ICP."""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import filter as F
from dicp_amd.filter import radius_outlier_removal, select_rows, statistical_outlier_removal
from dicp_amd.ICP import ICP
from dicp_amd.knn import knn_points
from dicp_amd.normals import estimate_normals
from dicp_amd.voxel import voxel_downsample

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref as fr  # noqa: E402
from ball_ref import ball_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
T = F.SELECT_TILE


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows_dev(rows):
    return None if rows is None else torch.tensor(list(rows), dtype=torch.int32).cuda()


# ------------------------------------------------------------------ 1. select_rows against the reference
def _hold_select(pts, mask, rows, seed=0):
    """one batch (N, m, c) with its mask (N, m) and row counts (or None): out, rows_out, index and the gradient, bit for bit.  The rows at
    and past rows[b] hold NaN and a True mask; the cotangent holds NaN on the output's pad rows."""
    N, m, c = pts.shape
    pts, mask = pts.copy(), mask.copy()
    refs = []
    for b in range(N):
        mb = m if rows is None else rows[b]
        pts[b, mb:] = np.nan
        mask[b, mb:] = True
        refs.append(fr.select_ref(pts[b], mask[b], mb))
    g = np.random.default_rng(seed).standard_normal((N, m, c)).astype(pts.dtype)
    for b in range(N):
        g[b, refs[b][1]:] = np.nan
    x = _dev(pts).requires_grad_(True)
    out, rows_out, index = select_rows(x, _dev(mask), rows=_rows_dev(rows), return_index=True)
    assert out.shape == (N, m, c) and out.dtype == x.dtype and rows_out.shape == (N,) and rows_out.dtype == torch.int32
    assert index.shape == (N, m) and index.dtype == torch.int64
    out.backward(_dev(g))
    o, r, ix, gx = _np(out), _np(rows_out), _np(index), _np(x.grad)
    assert not np.isnan(o).any() and not np.isnan(gx).any()
    for b in range(N):
        what = (N, m, c, b, rows)
        assert r[b] == refs[b][1], what
        assert np.array_equal(ix[b], refs[b][2]), what
        assert fr.same_bits(o[b], refs[b][0]), what
        assert fr.same_bits(gx[b], fr.select_grad_ref(g[b], refs[b][3])), what
    return out, rows_out, index, x.grad


def _masks(N, m, rng):
    """name -> (N, m) bool"""
    first, last, alt = np.zeros((N, m), bool), np.zeros((N, m), bool), np.zeros((N, m), bool)
    first[:, 0], last[:, -1], alt[:, ::2] = True, True, True
    dens = np.stack([rng.random(m) < d for d in ([0.05, 0.5, 0.95] * N)[:N]])
    return {"none": np.zeros((N, m), bool), "all": np.ones((N, m), bool), "first": first, "last": last, "alternating": alt,
            "random": rng.random((N, m)) < 0.5, "densities": dens}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [1, 3, 4, 6, 7])
def test_select_rows(c, dtype):
    rng = np.random.default_rng(c)
    for m in (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3):
        mid = max(1, m // 2) if m <= T else T + (m - T) // 2                       # inside a tile
        for N in (1, 3):
            pts = rng.standard_normal((N, m, c)).astype(dtype)
            row_sets = [[0], [1], [mid], [m], None] if N == 1 else [[0, mid, m], [m, 1, mid], None]
            for name, mask in _masks(N, m, rng).items():
                for rows in row_sets:
                    _hold_select(pts, mask, rows)


def test_select_rows_more_tiles_than_scan_threads():
    m = (F.SELECT_SCAN_THREADS + 2) * T + 5
    rng = np.random.default_rng(5)
    pts = rng.standard_normal((1, m, 3)).astype(np.float32)
    mask = rng.random((1, m)) < 0.5
    a = _hold_select(pts, mask, [m - 3])
    b = _hold_select(pts, mask, [m - 3])
    assert all(torch.equal(p, q) for p, q in zip(a, b))                    # two runs: equal bytes
    assert int(a[1][0]) > F.SELECT_SCAN_THREADS * T // 4


@pytest.mark.parametrize("dtype", DTYPES)
def test_select_rows_forms(dtype):
    rng = np.random.default_rng(8)
    lens = [T + 7, 1, 300]
    clouds = [rng.standard_normal((n, 4)).astype(dtype) for n in lens]
    masks = [rng.random(n) < 0.6 for n in lens]
    masks[1][:] = False
    refs = [fr.select_ref(p, k) for p, k in zip(clouds, masks)]
    # lists
    xs = [_dev(p).requires_grad_(True) for p in clouds]
    out, rows_out, index = select_rows(xs, [_dev(k) for k in masks], return_index=True)
    assert isinstance(out, list) and len(out) == 3 and len(rows_out) == 3 and rows_out[0].dim() == 0
    sum(o.sum() for o in out).backward()
    for b in range(3):
        n = refs[b][1]
        assert out[b].shape == (n, 4) and index[b].shape == (n,) and int(rows_out[b]) == n
        assert fr.same_bits(_np(out[b]), refs[b][0][:n]) and np.array_equal(_np(index[b]), refs[b][2][:n])
        assert np.array_equal(_np(xs[b].grad), np.repeat(masks[b][:, None], 4, 1).astype(dtype))
    # a single cloud; without a gradient and without the index
    out1, rows1 = select_rows(_dev(clouds[0]), _dev(masks[0]))
    assert out1.shape == (refs[0][1], 4) and rows1.dim() == 0 and int(rows1) == refs[0][1] and fr.same_bits(_np(out1), refs[0][0][:refs[0][1]])
    out1, rows1, index1 = select_rows(_dev(clouds[1]), _dev(masks[1]), return_index=True)
    assert out1.shape == (0, 4) and int(rows1) == 0 and index1.shape == (0,)
    # CPU tensors: computed on the GPU, returned on the CPU -- every form
    xc = torch.from_numpy(clouds[2]).requires_grad_(True)
    oc, rc, ic = select_rows(xc, torch.from_numpy(masks[2]), return_index=True)
    assert not oc.is_cuda and not rc.is_cuda and not ic.is_cuda and fr.same_bits(oc.detach().numpy(), refs[2][0][:refs[2][1]])
    oc.sum().backward()
    assert not xc.grad.is_cuda and np.array_equal(xc.grad.numpy(), np.repeat(masks[2][:, None], 4, 1).astype(dtype))
    pad = np.zeros((2, 300, 4), dtype)
    pad[0], pad[1, :200] = clouds[2], clouds[2][:200]
    mk = np.stack([masks[2], masks[2]])
    ob, rb, ib = select_rows(torch.from_numpy(pad), torch.from_numpy(mk), rows=torch.tensor([300, 200]), return_index=True)
    r1 = fr.select_ref(pad[1], mk[1], 200)
    assert not ob.is_cuda and ob.shape == (2, 300, 4) and list(rb) == [refs[2][1], r1[1]]
    assert fr.same_bits(ob[0].numpy(), refs[2][0]) and fr.same_bits(ob[1].numpy(), r1[0]) and np.array_equal(ib[1].numpy(), r1[2])
    ol, rl = select_rows([torch.from_numpy(p) for p in clouds], [torch.from_numpy(k) for k in masks])
    assert all(not o.is_cuda for o in ol) and [o.shape[0] for o in ol] == [r[1] for r in refs]


# ------------------------------------------------------------------ 2. no host synchronisation
def test_no_host_synchronisation():
    rng = np.random.default_rng(2)
    base = _dev(rng.random((2, 3000, 3)).astype(np.float32))
    mask = _dev(rng.random((2, 3000)) < 0.7)
    rd = torch.tensor([3000, 2500], dtype=torch.int32).cuda()

    def run():
        xd = base.clone().requires_grad_(True)
        a = select_rows(xd, mask, rows=rd, return_index=True)
        b = radius_outlier_removal(xd, 0.08, 4, rows=rd, return_mask=True, return_index=True)
        c = statistical_outlier_removal(xd, k=8, std_ratio=1.0, rows=rd, return_mask=True, return_index=True, return_mean_distance=True, return_stats=True)
        (a[0].sum() + b[0].sum() + c[0].sum()).backward()
        return a, b, c, xd.grad
    run()                                                   # (the library is loaded, the allocator is warm)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a, b, c, g = run()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for outs in (a, b, c):
        assert 0 < int(outs[1].min()) and int(outs[1].max()) < 3000
    assert torch.isfinite(g).all() and float(g.max()) == 3.0


# ------------------------------------------------------------------ 3. statistical_outlier_removal against the reference
def _hold_stat(x, k, ratio, rows=None):
    """x (N, m, c): every output of both methods against the reference evaluated on the d2 / idx that knn_points returns for x"""
    N, m, c = x.shape
    xd, rd = _dev(x), _rows_dev(rows)
    d2, idx = knn_points(xd, xd, k + 1, x_rows=rd, y_rows=rd)
    d2, idx = _np(d2), _np(idx)
    outs = {}
    for method in ("grid", "walk"):
        outs[method] = statistical_outlier_removal(xd, k=k, std_ratio=ratio, rows=rd, method=method, return_mask=True, return_index=True,
                                                   return_mean_distance=True, return_stats=True)
    assert all(torch.equal(a, b) or (a.dtype.is_floating_point and fr.same_bits(_np(a), _np(b))) for a, b in zip(outs["grid"], outs["walk"]))
    out, rows_out, mask, index, md, stats = outs["grid"]
    assert out.shape == (N, m, c) and mask.shape == (N, m) and mask.dtype == torch.bool and md.shape == (N, m) and md.dtype == torch.float64
    assert stats.shape == (N, 3) and stats.dtype == torch.float64 and index.shape == (N, m) and rows_out.dtype == torch.int32
    refs = []
    for b in range(N):
        mb = m if rows is None else rows[b]
        r_md, r_stats, r_mask = fr.outlier_ref(d2[b], idx[b], k, ratio, rows=mb)
        what = (m, k, b, rows)
        assert fr.same_bits(_np(md[b]), r_md), what
        assert fr.same_bits(_np(stats[b]), r_stats), (what, _np(stats[b]), r_stats)
        assert np.array_equal(_np(mask[b]), r_mask), what
        r_out, r_n, r_index, _ = fr.select_ref(x[b], r_mask, mb)
        assert int(rows_out[b]) == r_n and np.array_equal(_np(index[b]), r_index) and fr.same_bits(_np(out[b]), r_out), what
        refs.append((r_md, r_stats, r_mask))
    return refs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 8, 31])
def test_statistical_sizes(k, dtype):
    rng = np.random.default_rng(k)
    for m in sorted({1, 2, k, k + 1, 65, 4097}):
        x = rng.random((1, m, 3)).astype(dtype)
        if m >= 65:
            x[0, ::29] += dtype(3.0) + dtype(3.0) * rng.random((len(x[0, ::29]), 3)).astype(dtype)     # rows far from the cube
        refs = _hold_stat(x, k, 2.0)
        if m == 1:
            assert not refs[0][2].any() and np.isnan(refs[0][1][0])
        if m >= 65:
            assert 0 < refs[0][2].sum() < m


@pytest.mark.parametrize("dtype", DTYPES)
def test_statistical_duplicates_and_non_finite_rows(dtype):
    rng = np.random.default_rng(4)
    m = 3000
    x = rng.random((3, m, 4)).astype(dtype)
    dup = rng.choice(m - 1, m // 100, replace=False)
    x[0, dup + 1] = x[0, dup]                                          # 1 % exact duplicates
    x[1, 100:140, :3] = x[1, 100, :3]                                  # 40 copies of one point: a copy is not in its own list
    x[2, [5, 77, 900], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    refs = _hold_stat(x, 8, 1.5)
    assert np.isinf(refs[2][0][[5, 77, 900]]).all() and not refs[2][2][[5, 77, 900]].any()
    assert (refs[1][0][100:140] == 0).all()                            # their 8 nearest are other copies
    refs = _hold_stat(x, 31, 1.5)
    assert (refs[1][0][100:140] == 0).all()
    # ragged, with an empty cloud and a cloud of one row
    refs = _hold_stat(x, 8, 2.0, rows=[2500, 0, 1])
    assert not refs[1][2].any() and not refs[2][2].any() and np.isnan(refs[1][1][0]) and refs[0][2][:2500].any() and not refs[0][2][2500:].any()


def test_statistical_drops_planted_outliers_and_keeps_a_lattice():
    g = np.arange(8, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    k = 3                                                              # every lattice row, a corner too, has 3 rows at distance 1
    alone = _hold_stat(lattice[None], k, 2.0)[0]
    assert (alone[0] == 1.0).all() and list(alone[1]) == [1.0, 0.0, 1.0] and alone[2].all()      # the lattice alone: md = thr, all kept
    far = np.array([[60, 0, 0], [0, -70, 0], [0, 0, 90], [-50, 40, 0], [30, 30, 80]], dtype=np.float32)
    x = np.concatenate([lattice[:200], far[:2], lattice[200:], far[2:]])[None]
    planted = np.zeros(x.shape[1], bool)
    planted[[200, 201, -3, -2, -1]] = True
    ref = _hold_stat(x, k, 2.0)[0]
    assert np.array_equal(ref[2], ~planted)
    out, rows_out = statistical_outlier_removal(_dev(x[0]), k=k, std_ratio=2.0)
    assert int(rows_out) == 512 and np.array_equal(_np(out), lattice)


# ------------------------------------------------------------------ 4. radius_outlier_removal against the reference
def _hold_radius(x, radius, min_neighbors, rows=None):
    N, m, c = x.shape
    out, rows_out, mask, index = radius_outlier_removal(_dev(x), radius, min_neighbors, rows=_rows_dev(rows), return_mask=True, return_index=True)
    refs = []
    for b in range(N):
        mb = m if rows is None else rows[b]
        counts = ball_ref(x[b], x[b], radius, 1, x_rows=mb, y_rows=mb)[2]
        r_mask = counts >= min_neighbors
        r_out, r_n, r_index, _ = fr.select_ref(x[b], r_mask, mb)
        assert np.array_equal(_np(mask[b]), r_mask), (b, rows)
        assert int(rows_out[b]) == r_n and np.array_equal(_np(index[b]), r_index) and fr.same_bits(_np(out[b]), r_out), (b, rows)
        refs.append((counts, r_mask))
    return refs, out, rows_out


@pytest.mark.parametrize("dtype", DTYPES)
def test_radius_outlier_removal(dtype):
    g = np.arange(7, dtype=dtype)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    # the lattice on the bound: the radius is inclusive, a row counts itself -- 4 at a corner, 5 on an edge, 6 on a face, 7 inside
    refs, _, rows_out = _hold_radius(lattice[None], 1.0, 6)
    assert sorted(set(refs[0][0])) == [4, 5, 6, 7] and int(rows_out[0]) == 5 ** 3 + 6 * 25
    rng = np.random.default_rng(6)
    x = rng.random((2, 1500, 5)).astype(dtype)
    x[0, [3, 40, 1400], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    refs, _, rows_out = _hold_radius(x, 0.07, 3, rows=[1500, 1100])
    assert 0 < int(rows_out[0]) < 1500 and 0 < int(rows_out[1]) < 1100
    # min_neighbors = 1: only the non-finite rows go
    refs, _, rows_out = _hold_radius(x, 0.07, 1)
    assert list(np.flatnonzero(~refs[0][1])) == [3, 40, 1400] and refs[1][1].all() and list(_np(rows_out)) == [1497, 1500]
    # a value above every count: nothing is kept
    refs, out, rows_out = _hold_radius(x, 0.07, 1501)
    assert list(_np(rows_out)) == [0, 0] and not _np(out).any()
    # gradients reach the kept rows only
    xd = _dev(x).requires_grad_(True)
    out, rows_out, mask = radius_outlier_removal(xd, 0.07, 3, return_mask=True)
    out.sum().backward()
    assert torch.equal(xd.grad, mask[..., None].expand_as(xd).to(xd.dtype))


# ------------------------------------------------------------------ 5. the chain voxel -> filter -> normals -> ICP
def _chain(raw0, rows):
    raw = raw0.clone().requires_grad_(True)
    cent, crow, inverse = voxel_downsample(raw, 0.05, rows=rows, return_inverse=True)
    cloud, frow, mask = statistical_outlier_removal(cent, k=8, std_ratio=2.0, rows=crow, return_mask=True)
    nrm = estimate_normals(cloud, k=12, method="grid", rows=frow, deterministic=True)
    target = torch.cat((cloud, nrm), -1)
    src = (cloud.detach() * 1.01 + 0.01).contiguous()
    T0 = torch.eye(4, dtype=raw.dtype, device="cuda").repeat(raw.shape[0], 1, 1)
    icp = ICP(icp_type="pt2pl", differentiable=True, max_iterations=3, tolerance=1e-12)
    icp.deterministic = True
    out = icp.icp(src, target, T0, source_rows=frow, target_rows=frow)
    out["T"].sum().backward()
    return raw.grad, cent.detach(), crow, inverse, cloud.detach(), frow, mask, nrm.detach()


def test_chain_voxel_filter_normals_icp():
    rng = np.random.default_rng(12)
    xy = rng.random((2, 4000, 2)) * 2.0
    z = 0.3 * np.sin(2.0 * xy[..., :1]) * np.cos(xy[..., 1:]) + 0.003 * rng.standard_normal((2, 4000, 1))
    raw_np = np.concatenate([xy, z], -1).astype(np.float32)
    raw_np[:, ::400] += np.float32(2.0) + rng.random((2, 10, 3)).astype(np.float32)          # stray points off the surface
    raw0 = _dev(raw_np)
    rows = torch.tensor([4000, 3500], dtype=torch.int32).cuda()
    g, cent, crow, inverse, cloud, frow, mask, nrm = _chain(raw0, rows)
    g2 = _chain(raw0, rows)[0]
    assert torch.equal(g, g2)                                              # deterministic operators: the same bytes twice
    assert torch.isfinite(g).all() and (g != 0).any()
    c_np, m_np, inv = _np(cent), _np(mask), _np(inverse)
    host = np.zeros_like(c_np)
    for b in range(2):
        r_out, r_n, _, _ = fr.select_ref(c_np[b], m_np[b], int(crow[b]))
        assert r_n == int(frow[b]) and 500 < r_n < int(crow[b])            # the filter dropped something
        host[b] = r_out
        assert fr.same_bits(_np(cloud[b]), r_out)
        # a raw row whose voxel's centroid was dropped (or that has no voxel) gets exactly 0
        gone = (inv[b] < 0) | ~m_np[b][np.maximum(inv[b], 0)]
        assert gone[:int(rows[b])].sum() > (inv[b][:int(rows[b])] < 0).sum() and not _np(g[b])[gone].any()
        assert _np(g[b])[~gone].any()
    nrm_host = estimate_normals(_dev(host), k=12, method="grid", rows=frow, deterministic=True)
    assert fr.same_bits(_np(nrm), _np(nrm_host)) and (nrm != 0).any()
