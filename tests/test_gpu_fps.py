"""sample_farthest_points on the MI355X against its definition (dicp_amd/fps.py): indices, picked rows, k_eff and distances EXACTLY as the numpy
restatement tests/fps_ref.py gives them (tests/test_fps_host.py holds that restatement to the kernels' own header without a GPU) -- both
kernel forms at every size where they change path, ties and duplicates, rows that are no candidates, overflow, every input form, the
gradient, and the voxel_downsample -> sample_farthest_points -> ICP chain.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import fps
from dicp_amd.fps import sample_farthest_points
from dicp_amd.ICP import ICP
from dicp_amd.synthetic import make_pairs
from dicp_amd.voxel import voxel_downsample

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fps_clouds as fc  # noqa: E402
from fps_ref import fps_ref  # noqa: E402

pytestmark = pytest.mark.gpu

T = fps.T
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
DTYPES = [np.float32, np.float64]
_REFS = {}


def _ref(name, p, k, start):
    """the reference of the named cloud, computed once per (cloud, start) at the largest k asked so far: a pick does not depend on k, so a
    shorter call is a prefix (of its first n entries; the rest are unused slots)"""
    key = (name, p.dtype.str, int(start))
    if key not in _REFS or _REFS[key][0] < k:
        _REFS[key] = (k,) + fps_ref(p, k, start=start)
    _, idx, dist, _ = _REFS[key]
    keff = int((idx[:k] >= 0).sum())
    return idx[:k], dist[:k], keff


def _pad(clouds):
    """a list of (n_b, c) numpy clouds -> ((N, n, c) batch whose pad rows hold far finite points that would win any pick, rows)"""
    n = max(max(p.shape[0] for p in clouds), 1)
    c, dt = clouds[0].shape[1], clouds[0].dtype
    batch = np.random.default_rng(99).uniform(1e3, 2e3, (len(clouds), n, c)).astype(dt)
    for b, p in enumerate(clouds):
        batch[b, :p.shape[0]] = p
    return batch, [p.shape[0] for p in clouds]


def _call(clouds, k, starts, form):
    batch, rows = _pad(clouds)
    start = starts if isinstance(starts, int) else torch.tensor(starts, dtype=torch.int64).cuda()
    pts, idx, keff, dist = sample_farthest_points(torch.from_numpy(batch).cuda(), k, rows=torch.tensor(rows, dtype=torch.int32).cuda(), start=start,
                                                  return_rows=True, return_distances=True, _form=form)
    N, c = len(clouds), clouds[0].shape[1]
    assert pts.shape == (N, k, c) and idx.shape == (N, k) and keff.shape == (N,) and dist.shape == (N, k)
    assert pts.dtype == TORCH[clouds[0].dtype.type] and idx.dtype == torch.int64 and keff.dtype == torch.int32 and dist.dtype == pts.dtype
    return pts.cpu().numpy(), idx.cpu().numpy(), keff.cpu().numpy(), dist.cpu().numpy()


def _check(names, clouds, k, starts=0, forms=(None,)):
    """the GPU call on the ragged batch of the clouds, every cloud against the reference; with several forms, the forms against each other too"""
    outs = [_call(clouds, k, starts, f) for f in forms]
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert a.tobytes() == b.tobytes()
    pts, idx, keff, dist = outs[0]
    for b, (name, p) in enumerate(zip(names, clouds)):
        s = starts if isinstance(starts, int) else starts[b]
        ri, rd, rk = _ref(name, p, k, s)
        assert keff[b] == rk, (name, keff[b], rk)
        assert np.array_equal(idx[b], ri), (name, np.flatnonzero(idx[b] != ri)[:5])
        assert dist[b].tobytes() == rd.tobytes(), name
        want = np.zeros((k, p.shape[1]), dtype=p.dtype)
        want[:rk] = p[ri[:rk]]
        assert pts[b].tobytes() == want.tobytes(), name                                       # bit for bit; zero rows past k_eff
        assert (idx[b, rk:] == -1).all() and np.isposinf(dist[b, rk:]).all()


def _sizes(dtype):
    NR = fps.NR[TORCH[dtype]]
    return [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, NR - 1, NR]


def _size_clouds(dtype):
    return (["rand%d" % n for n in _sizes(dtype)], [fc.random_cloud(n, 3, dtype, 100 + i) for i, n in enumerate(_sizes(dtype))])


def _starts(kind, sizes):
    rng = np.random.default_rng(7)
    return {"zero": 0, "last": [n - 1 for n in sizes], "past": [n + 5 for n in sizes], "tensor": [int(rng.integers(0, 3 * n)) for n in sizes]}[kind]


# ------------------------------------------------------------------ 1. the resident form
@pytest.mark.parametrize("kind", ["zero", "last", "past", "tensor"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_resident_form_matches_reference(dtype, kind):
    names, clouds = _size_clouds(dtype)
    starts = _starts(kind, _sizes(dtype))
    for k in (513, 64, 2, 1):
        _check(names, clouds, k, starts, forms=("resident", None))                            # (unforced: the same form, by size)


@pytest.mark.parametrize("dtype", DTYPES)
def test_resident_form_takes_whole_clouds(dtype):
    """k = n: every row is picked, as one cloud per call (the instantiations of 1, 2 and 4 rows a thread)"""
    names, clouds = _size_clouds(dtype)
    for name, p in zip(names, clouds):
        if p.shape[0] <= 2 * T + 1:
            _check([name], [p], p.shape[0], 0, forms=("resident",))
            _check([name], [p], p.shape[0] + 3, p.shape[0] // 2, forms=("resident",))


# ------------------------------------------------------------------ 2. ties and duplicates
def _tie_clouds(dtype):
    return (["lattice300", "lattice5000", "repeated200", "grid17"],
            [fc.lattice_cloud(300, dtype), fc.lattice_cloud(5000, dtype), fc.repeated_point(200, dtype), fc.grid_cloud(17, dtype)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_and_duplicates(dtype):
    for name, p in zip(*_tie_clouds(dtype)):
        n = p.shape[0]
        _check([name], [p], n, 3, forms=("resident", "streamed"))
        idx = _ref(name, p, n, 3)[0]
        assert np.array_equal(np.sort(idx), np.arange(n))                                     # the reference's permutation


# ------------------------------------------------------------------ 3. rows that are no candidates
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_candidates(dtype):
    bad = fc.nonfinite_cloud(700, dtype)
    none = np.full((50, 3), np.nan, dtype=dtype)
    none[::3] = np.inf
    none[1::3, 1] = -np.inf
    ok = fc.random_cloud(300, 3, dtype, 40)
    empty = ok[:0]
    names, clouds = ["bad", "none", "ok", "empty", "bad"], [bad, none, ok, empty, bad]
    assert not np.isfinite(bad[5]).all() and not np.isfinite(bad[-9:]).all(1).any()
    for starts in ([5, 0, 0, 0, 699], [0, 7, 299, 3, 695]):                                   # starts on non-finite rows, wrapping past the last rows
        for k in (800, 64):                                                                   # above the candidate count, and below
            _check(names, clouds, k, starts, forms=("resident", "streamed"))
    assert _ref("bad", bad, 800, 5)[2] == np.isfinite(bad).all(1).sum() < 700 and _ref("none", none, 800, 0)[2] == 0


# ------------------------------------------------------------------ 4. overflow and far clouds
def test_overflow_and_far_clouds():
    over, sphere = fc.overflow_cloud(), fc.sphere_cloud()
    assert np.isposinf(_ref("overflow", over, 500, 0)[1][1:]).sum() > 10
    _check(["overflow"], [over], 500, 0, forms=("resident", "streamed"))
    _check(["sphere"], [sphere], 400, 0, forms=("resident", "streamed"))
    s64 = sphere.astype(np.float64)
    _check(["sphere"], [s64], 400, 0, forms=("resident", "streamed"))
    assert (_ref("sphere", sphere, 400, 0)[0] != _ref("sphere", s64, 400, 0)[0]).any()          # the two dtypes are told apart


# ------------------------------------------------------------------ 5. the streamed form
@pytest.mark.parametrize("dtype", DTYPES)
def test_streamed_form_matches_reference(dtype):
    S = fps.STREAM_ROWS
    sizes = [1, 65, S - 1, S, S + 1, 5000]
    names, clouds = ["srand%d" % n for n in sizes], [fc.random_cloud(n, 3, dtype, 200 + i) for i, n in enumerate(sizes)]
    for k, starts in ((64, [n + 5 for n in sizes]), (1, 0), (65, [n - 1 for n in sizes])):
        _check(names, clouds, k, starts, forms=("streamed", "resident"))
    for name, p in zip(names, clouds):                                                        # one cloud per call: the workgroup count changes at S
        _check([name], [p], min(p.shape[0], 65), 2, forms=("streamed",))


@pytest.mark.parametrize("dtype", DTYPES)
def test_large_clouds_take_the_streamed_form(dtype):
    NR = fps.NR[TORCH[dtype]]
    for n in (NR + 1, NR + T + 1):
        p = fc.random_cloud(n, 3, dtype, n)
        _check(["big%d" % n], [p], 64, n - 1, forms=(None, "streamed"))
        with pytest.raises(ValueError):
            sample_farthest_points(torch.from_numpy(p).cuda(), 64, _form="resident")


# ------------------------------------------------------------------ 6. every input form
@pytest.mark.parametrize("dtype", DTYPES)
def test_input_forms(dtype):
    tdt = TORCH[dtype]
    for c in (3, 4, 6, 9):
        clouds = [fc.random_cloud(n, c, dtype, 300 + c + n) for n in (400, 37, 250)]
        names = ["c%d_%d" % (c, p.shape[0]) for p in clouds]
        _check(names, clouds, 50, [9, 2, 777], forms=("resident", "streamed"))               # device rows; the extra columns arrive unchanged
        k = 50
        refs = [_ref(nm, p, k, 0) for nm, p in zip(names, clouds)]
        # a list of clouds
        lp, li, lr, ld = sample_farthest_points([torch.from_numpy(p).cuda() for p in clouds], k, return_rows=True, return_distances=True)
        for b, p in enumerate(clouds):
            m = min(k, p.shape[0])
            assert lp[b].shape == (m, c) and li[b].shape == (m,) and ld[b].shape == (m,) and int(lr[b]) == refs[b][2] == m
            assert np.array_equal(li[b].cpu().numpy(), refs[b][0][:m]) and np.array_equal(lp[b].cpu().numpy(), p[refs[b][0][:m]])
        # one cloud, on the device and from the CPU
        for dev in ("cuda", "cpu"):
            x = torch.from_numpy(clouds[0]).to(dev)
            sp, si, sr, sd = sample_farthest_points(x, k, return_rows=True, return_distances=True)
            assert sp.device.type == si.device.type == sr.device.type == sd.device.type == dev
            assert sp.shape == (k, c) and si.shape == (k,) and sr.dim() == 0 and int(sr) == k and sp.dtype == tdt
            assert np.array_equal(si.cpu().numpy(), refs[0][0]) and sd.cpu().numpy().tobytes() == refs[0][1].tobytes()
            assert np.array_equal(sp.cpu().numpy(), clouds[0][refs[0][0]])
            assert len(sample_farthest_points(x, k)) == 2 and len(sample_farthest_points(x, k, return_distances=True)) == 3
        # a padded batch without rows, with CPU rows, and a non-contiguous view
        full = np.stack([fc.random_cloud(120, c, dtype, 350 + c + b) for b in range(3)])
        fr = [fps_ref(full[b], 20)[0] for b in range(3)]
        bi = sample_farthest_points(torch.from_numpy(full).cuda(), 20)[1]
        assert np.array_equal(bi.cpu().numpy(), np.stack(fr))
        cut = [fps_ref(full[b], 20, rows=r, start=4)[0] for b, r in enumerate((120, 7, 0))]
        ci = sample_farthest_points(torch.from_numpy(full).cuda(), 20, rows=torch.tensor([120, 7, 0]), start=4)[1]
        assert np.array_equal(ci.cpu().numpy(), np.stack(cut))
        wide = torch.from_numpy(np.concatenate((full, full), axis=2)).cuda()
        view = wide[:, ::2, 1:c + 1]
        assert not view.is_contiguous()
        vp, vi = sample_farthest_points(view, 20)
        vn = view.cpu().numpy()
        assert all(np.array_equal(vi[b].cpu().numpy(), fps_ref(vn[b], 20)[0]) for b in range(3))
        assert np.array_equal(vp.cpu().numpy(), np.stack([vn[b][vi[b].cpu().numpy()] for b in range(3)]))
    # a batch without any row
    ep, ei, er = sample_farthest_points(torch.zeros((2, 0, 3), dtype=tdt).cuda(), 4, return_rows=True)
    assert ep.shape == (2, 4, 3) and (ep == 0).all() and (ei == -1).all() and (er == 0).all()


# ------------------------------------------------------------------ 7. the gradient
@pytest.mark.parametrize("form", ["resident", "streamed"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gradient_is_the_scatter_of_the_cotangent(dtype, form, monkeypatch):
    calls = []
    real = fps._scatter
    monkeypatch.setattr(fps, "_scatter", lambda *a: (calls.append(1), real(*a))[1])
    for c in (3, 6):
        clouds = [fc.random_cloud(n, c, dtype, 400 + n) for n in (500, 30, 260, 1)]
        batch, rows = _pad(clouds)
        rows_t = torch.tensor(rows, dtype=torch.int32).cuda()
        k = 64
        G = torch.from_numpy(fc.random_cloud(len(clouds) * k, c, dtype, 77).reshape(len(clouds), k, c)).cuda()
        grads = []
        for _ in range(2):
            x = torch.from_numpy(batch).cuda().requires_grad_(True)
            pts, idx, keff, dist = sample_farthest_points(x, k, rows=rows_t, start=3, return_rows=True, return_distances=True, _form=form)
            assert pts.requires_grad and not idx.requires_grad and not keff.requires_grad and not dist.requires_grad
            n_before = len(calls)
            pts.backward(G)
            assert len(calls) == n_before + 1
            grads.append(x.grad.clone())
        want = torch.zeros_like(grads[0])
        idx_h, keff_h = idx.cpu().numpy(), keff.cpu().numpy()
        assert list(keff_h) == [min(k, r) for r in rows]
        for b in range(len(clouds)):
            want[b, idx_h[b, :keff_h[b]]] = G[b, :keff_h[b]]                                  # slots past k_eff contribute nothing
        assert torch.equal(grads[0], want) and torch.equal(grads[0], grads[1])                # bit for bit, and from run to run
        assert (want != 0).any()
    # without requires_grad nothing of the backward runs or is recorded
    n_before = len(calls)
    pts = sample_farthest_points(torch.from_numpy(batch).cuda(), k, rows=rows_t, _form=form)[0]
    assert not pts.requires_grad and pts.grad_fn is None and len(calls) == n_before
    # through the CPU round trip too
    xc = torch.from_numpy(clouds[0]).requires_grad_(True)
    pc, ic = sample_farthest_points(xc, 8, _form=form)
    pc.sum().backward()
    wc = torch.zeros_like(xc)
    wc[ic] = 1
    assert torch.equal(xc.grad, wc)


# ------------------------------------------------------------------ 8. the chain
def test_voxel_fps_icp_chain():
    src, tgt = make_pairs(4, 3000, 3000, seed=5, dtype=torch.float32)
    scan = src.cuda().requires_grad_(True)
    tgt = tgt.cuda()
    T0 = torch.eye(4).repeat(4, 1, 1).cuda()
    cent, rs = voxel_downsample(scan, 1.0)
    pts, idx, kr = sample_farthest_points(cent, 256, rows=rs, return_rows=True)
    assert pts.shape == (4, 256, 3) and (kr == 256).all()
    icp = ICP(icp_type="pt2pt", differentiable=True, max_iterations=5, tolerance=1e-6)
    out = icp.icp(pts, tgt, T0, source_rows=kr)
    out["T"].sum().backward()
    assert torch.isfinite(out["T"]).all() and torch.isfinite(scan.grad).all() and (scan.grad != 0).any()
    gathered = torch.gather(cent, 1, idx[..., None].expand(-1, -1, 3))
    assert torch.equal(gathered, pts)
    out2 = icp.icp(gathered, tgt, T0, source_rows=kr)
    assert torch.equal(out2["T"], out["T"])                                                   # the pose of points[idx] gathered with torch, bit for bit


# ------------------------------------------------------------------ 9. start="random"
def test_random_start():
    clouds = torch.from_numpy(np.stack([fc.random_cloud(300, 3, np.float32, 500 + b) for b in range(5)])).cuda()
    rows = torch.tensor([300, 17, 150, 1, 299])
    torch.manual_seed(1234)
    a = sample_farthest_points(clouds, 16, rows=rows, start="random")[1]
    torch.manual_seed(1234)
    b = sample_farthest_points(clouds, 16, rows=rows, start="random")[1]
    torch.manual_seed(1234)
    draw = torch.randint(0, 2 ** 62, (5,), dtype=torch.int64)
    assert torch.equal(a, b) and torch.equal(a[:, 0].cpu(), draw % rows)
    c = sample_farthest_points(clouds, 16, rows=rows, start="random")[1]                       # the generator has moved on
    assert not torch.equal(a[:, 0], c[:, 0])
