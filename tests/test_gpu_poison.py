"""No returned byte depends on what an uninitialised buffer held: every front end of dicp_amd, forward and backward, run clean, with every
torch.empty / torch.empty_like buffer filled with 0xFF (NaN, -1, true) and with 0xFE (about -1.7e38 / -5.3e303, large negative integers) --
tests/poison.py.  Outputs the docstrings call bit-reproducible or stored once, and every integer, bool and index output, give the same bytes in
the three runs.  The gradients the README says are added with float atomics stay finite wherever the clean run is finite and are held to the
deterministic=True result (the float64 oracle for the ICP loop) with the bounds their own GPU tests derive -- restated here, none fitted.

Inputs: ragged batches of three clouds, one of them with 0 rows, NaN in the pad rows, six columns where the operator takes extra columns, a few
hundred rows (more than one tile and more than one wave, no more than a handful).  A probe builds its inputs once from fixed seeds, runs one
front-end call forward and, where gradients are offered, backward with a fixed random cotangent, and returns every tensor the user gets back."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ball_clouds as bc  # noqa: E402
import compat_cases as cc  # noqa: E402
import fpfh_cases as fc  # noqa: E402
import gumbel_ref as G  # noqa: E402
import icp_rows_ref as R  # noqa: E402
import inverse_ref as ir  # noqa: E402
import iss_cases as ic  # noqa: E402
import knn_det_ref as kr  # noqa: E402
import normals_det_ref as nr  # noqa: E402
import walk_layouts as wl  # noqa: E402
from poison import hold  # noqa: E402

from dicp_amd import _call, _lib, _loop, _ops  # noqa: E402
from dicp_amd.ICP import ICP  # noqa: E402
from dicp_amd.ball import ball_query  # noqa: E402
from dicp_amd.compat import correspondence_compatibility, prune_correspondences, second_order_compatibility  # noqa: E402
from dicp_amd.evaluate import evaluate_registration, information_matrix  # noqa: E402
from dicp_amd.filter import radius_outlier_removal, select_rows, statistical_outlier_removal  # noqa: E402
from dicp_amd.fpfh import compute_fpfh, fpfh_features  # noqa: E402
from dicp_amd.fps import sample_farthest_points  # noqa: E402
from dicp_amd.group import group_points, interpolate_features, invert_neighbors, pool_neighbors  # noqa: E402
from dicp_amd.iss import compute_iss_keypoints, iss_keypoints, iss_keypoints_ball, iss_saliency, iss_saliency_ball  # noqa: E402
from dicp_amd.knn import chamfer_distance, knn_points  # noqa: E402
from dicp_amd.match import knn_features, match_features, soft_match_features  # noqa: E402
from dicp_amd.normals import estimate_normals  # noqa: E402
from dicp_amd.register import (align_correspondences, consensus_correspondences, correspondence_residuals, gnc_correspondences,  # noqa: E402
                               ransac_correspondences)
from dicp_amd.synthetic import make_pairs  # noqa: E402
from dicp_amd.voxel import voxel_downsample  # noqa: E402
from oracle import dicp_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
ids = lambda d: np.dtype(d).name
N, NX, NY = 3, 300, 330
XR, YR = (300, 0, 211), (330, 170, 0)           # cloud 1 has no queries; cloud 2 has queries and no candidate: every slot empty
SR = (330, 0, 200)                              # one cloud's own row counts


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rows_t(rows):
    return torch.tensor(rows, dtype=torch.int32).cuda()


def cpu(**named):
    torch.cuda.synchronize()
    return {k: (v.detach().cpu() if v is not None else None) for k, v in named.items()}


def batch(n, rows, c, dtype, seed):
    """(N, n, c): ball_clouds.random_pair's unit-cube rows, random extra columns, NaN in every column of the rows at and past rows[b]"""
    out = np.full((len(rows), n, c), np.nan, dtype=dtype)
    for b, r in enumerate(rows):
        out[b, :r, :3] = bc.random_pair(n, n, dtype, seed=seed + b)[0][:r]
        out[b, :r, 3:] = np.random.default_rng(seed + 50 + b).standard_normal((r, c - 3)).astype(dtype)
    return out


def cot(shape, dtype, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(dtype)


# ------------------------------------------------------------------ knn_points, ball_query, chamfer_distance
def _neighbour_probe(op, dtype, c=6, **kw):
    k = kw["k"]
    X, Y, G = batch(NX, XR, c, dtype, 1), batch(NY, YR, c, dtype, 11), cot((N, NX, k), dtype, 21)

    def probe(**over):
        x, y = dev(X).requires_grad_(True), dev(Y).requires_grad_(True)
        out = op(x, y, x_rows=rows_t(XR), y_rows=rows_t(YR), **dict(kw, **over))
        torch.autograd.backward(out[0], dev(G))
        return cpu(d2=out[0], idx=out[1], counts=out[2] if len(out) > 2 else None, gx=x.grad, gy=y.grad)
    return probe, X, Y, G


def _gy_within_the_atomic_bound(det, X, Y, G, dtype):
    """test_gpu_knn_det.py's _hold: the atomic y-gradient within B + By (knn_det_ref.knn_det_bound) of the deterministic one; extra columns,
    pad rows and clouds without a live entry exactly 0"""
    def check(gy, outs):
        gy, idx, ref = gy.numpy(), outs["idx"].numpy(), det["gy"].numpy()
        assert np.array_equal(idx, det["idx"].numpy())
        for b in range(N):
            nb, mb = XR[b], YR[b]
            assert (gy[b, :, 3:] == 0).all() and (gy[b, mb:] == 0).all()
            if nb and mb:
                _, B, deg, By = kr.knn_det_bound(G[b, :nb], idx[b, :nb], X[b, :nb], Y[b, :mb], None, dtype)
                assert deg.max() > 1
                wl.assert_within(gy[b, :mb, :3], ref[b, :mb, :3].astype(np.longdouble), B + By, "atomic against deterministic, cloud %d" % b)
    return check


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("method", ["walk", "grid"])
def test_knn_points(method, det, k, dtype):
    probe, X, Y, G = _neighbour_probe(knn_points, dtype, k=k, method=method, deterministic=det)
    atomic = {} if det else {"gy": _gy_within_the_atomic_bound(probe(deterministic=True), X, Y, G, dtype)}
    clean = hold(probe, atomic=atomic, label="knn_points %s" % method)
    assert (clean["idx"][0] >= 0).all() and (clean["idx"][1:] == -1).all() and (clean["gx"][0] != 0).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
def test_ball_query(det, dtype):
    probe, X, Y, G = _neighbour_probe(ball_query, dtype, radius=0.25, k=8, return_counts=True, deterministic=det)
    atomic = {} if det else {"gy": _gy_within_the_atomic_bound(probe(deterministic=True), X, Y, G, dtype)}
    clean = hold(probe, atomic=atomic, label="ball_query")
    assert (clean["idx"][0] >= 0).any() and (clean["idx"][0] < 0).any() and clean["counts"][0].max() > 8 and (clean["counts"][1:] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("method", ["walk", "grid"])
def test_chamfer_distance(method, det, dtype):
    """reduction="none" under a random cotangent per cloud.  Cloud 1 is empty on both sides here (a non-empty side facing an empty cloud gives
    +inf, whose gradient is not a number the operator defines)."""
    xr, yr = (300, 0, 211), (330, 0, 170)
    X, Y, G = batch(NX, xr, 6, dtype, 2), batch(NY, yr, 6, dtype, 12), cot((N,), dtype, 22)

    def probe(deterministic=det):
        x, y = dev(X).requires_grad_(True), dev(Y).requires_grad_(True)
        per = chamfer_distance(x, y, x_rows=rows_t(xr), y_rows=rows_t(yr), reduction="none", method=method, deterministic=deterministic)
        per.backward(dev(G))
        return cpu(per=per, gx=x.grad, gy=y.grad)
    if det:
        hold(probe, label="chamfer %s" % method)
        return
    ref = probe(deterministic=True)
    u = wl.U[np.dtype(dtype)]

    def within(name, P, pr, Q, qr):
        """test_gpu_knn_det.py::test_chamfer_both_gradients: a cloud's gradient = its x-gradient as the query side (written once) + its atomic
        sum as the target side of the other search, one more addition"""
        def check(got, outs):
            got, want = got.numpy(), ref[name].numpy()
            for b in range(N):
                nb, mb = pr[b], qr[b]                       # this cloud's rows, the other cloud's (the queries of the search it is the target of)
                assert (got[b, nb:] == 0).all() and (got[b, :, 3:] == 0).all()
                if not (nb and mb):
                    continue
                A, Bc = Q[b, :mb, :3], P[b, :nb, :3]        # queries A, targets Bc
                _, io = wl.knn_oracle(A, Bc, 1)
                g = np.full((mb, 1), G[b] / dtype(mb), dtype=dtype)
                _, io_self = wl.knn_oracle(Bc, A, 1)
                gq = (2.0 * (G[b] / dtype(nb)).astype(np.float64) * (Bc.astype(np.float64) - A[io_self[:, 0]].astype(np.float64))).astype(dtype)
                _, Bd, _, By = kr.knn_det_bound(g, io, A, Bc, None, dtype)
                r = want[b, :nb, :3]
                wl.assert_within(got[b, :nb, :3], r.astype(np.longdouble), (Bd + By) * (1 + u) + 2 * u * (np.abs(r) + np.abs(gq) + Bd + By),
                                 "chamfer atomic %s cloud %d" % (name, b))
        return check
    hold(probe, atomic={"gx": within("gx", X, xr, Y, yr), "gy": within("gy", Y, yr, X, xr)}, label="chamfer %s" % method)


# ------------------------------------------------------------------ estimate_normals
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("method", ["walk", "grid"])
def test_estimate_normals(method, det, dtype):
    k = 8
    P, GN, GC = batch(NY, SR, 6, dtype, 3), cot((N, NY, 3), dtype, 23), cot((N, NY), dtype, 24)
    vp = torch.tensor([0.5, 0.5, 9.0], dtype=TORCH[dtype])

    def probe(deterministic=det, records=None):
        x = dev(P).requires_grad_(True)
        nrm, curv, nbr = estimate_normals(x, k=k, viewpoint=vp, rows=rows_t(SR), return_curvature=True, return_neighbors=True, method=method,
                                          deterministic=deterministic, _records=records)
        torch.autograd.backward([nrm, curv], [dev(GN), dev(GC)])
        return cpu(normals=nrm, curvature=curv, neighbours=nbr, grad=x.grad)
    if det:
        clean = hold(probe, label="normals %s" % method)
        assert (clean["grad"][0] != 0).any() and (clean["neighbours"][1] == -1).all()
        return
    recs = []
    ref = probe(deterministic=True, records=recs)
    rec, nbr = recs[0][0].cpu().numpy(), ref["neighbours"].numpy()
    u, ud = nr.U[dtype], 2.0 ** -53

    def check(grad, outs):
        """test_gpu_normals_det.py: |det - atomic| <= 2 (deg + 2) u_T (A + 8 u_double M) + 8 u_double M"""
        grad = grad.numpy()
        assert np.array_equal(outs["neighbours"].numpy(), nbr)
        for b in range(N):
            mb = SR[b]
            assert (grad[b, mb:] == 0).all() and (grad[b, :, 3:] == 0).all()
            if mb:
                off, slots = ir.invert_ref(nbr[b, :mb], mb, None)
                _, A, deg, M = nr.normals_det_bound(rec[b, :mb], nbr[b, :mb], None, off, slots, dtype)
                slack = 8 * ud * M * (1 + 2.0 ** -40)
                B2 = 2 * (deg + 2)[:, None] * u * (A + slack) + slack
                wl.assert_within(grad[b, :mb, :3], ref["grad"].numpy()[b, :mb, :3].astype(np.longdouble), B2, "normals atomic against det, cloud %d" % b)
    hold(probe, atomic={"grad": check}, label="normals %s" % method)


# ------------------------------------------------------------------ voxel_downsample, the filters, farthest-point sampling
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_voxel_downsample(dtype):
    P = batch(NY, SR, 6, dtype, 4)

    def probe():
        x = dev(P).requires_grad_(True)
        cen, rows_out, counts, inverse = voxel_downsample(x, 0.2, rows=rows_t(SR), min_points=2, return_counts=True, return_inverse=True)
        cen.backward(dev(cot(tuple(cen.shape), dtype, 25)))
        return cpu(centroids=cen, rows_out=rows_out, counts=counts, inverse=inverse, grad=x.grad)
    clean = hold(probe, label="voxel_downsample")
    assert clean["rows_out"][1] == 0 and 1 < clean["rows_out"][2] < clean["rows_out"][0] and (clean["inverse"] == -1).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("op", ["select", "radius", "statistical walk", "statistical grid"])
def test_filters(op, dtype):
    P = batch(NY, SR, 6, dtype, 5)
    M = np.random.default_rng(35).random((N, NY)) < 0.6

    def probe():
        x = dev(P).requires_grad_(True)
        mask = md = stats = None
        if op == "select":
            out, rows_out, index = select_rows(x, dev(M), rows=rows_t(SR), return_index=True)
        elif op == "radius":
            out, rows_out, mask, index = radius_outlier_removal(x, 0.25, 12, rows=rows_t(SR), return_mask=True, return_index=True)
        else:
            out, rows_out, mask, index, md, stats = statistical_outlier_removal(x, k=8, std_ratio=1.0, rows=rows_t(SR), method=op.split()[1], return_mask=True,
                                                                                return_index=True, return_mean_distance=True, return_stats=True)
        out.backward(dev(cot(tuple(out.shape), dtype, 26)))
        return cpu(out=out, rows_out=rows_out, index=index, mask=mask, mean_distance=md, stats=stats, grad=x.grad)
    clean = hold(probe, label=op)
    assert clean["rows_out"][1] == 0 and 0 < clean["rows_out"][2] < SR[2] and 0 < clean["rows_out"][0] < SR[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("form", ["resident", "streamed"])
def test_sample_farthest_points(form, dtype):
    P = batch(NY, SR, 6, dtype, 6)
    k = 210                                                 # more than cloud 2 holds: unused slots

    def probe():
        x = dev(P).requires_grad_(True)
        pts, idx, keff, dist = sample_farthest_points(x, k, rows=rows_t(SR), start=3, return_rows=True, return_distances=True, _form=form)
        pts.backward(dev(cot((N, k, 6), dtype, 27)))
        return cpu(pts=pts, idx=idx, k_eff=keff, distances=dist, grad=x.grad)
    clean = hold(probe, label="fps " + form)
    assert clean["k_eff"].tolist() == [210, 0, 200] and (clean["idx"][2, 200:] == -1).all()


# ------------------------------------------------------------------ invert_neighbors, group_points, pool_neighbors, interpolate_features
@functools.lru_cache(maxsize=None)
def _feature_case(dtype, it, C=5, k=8):
    """a table of C columns over the rows of batch Y and the neighbour lists of the queries X in it (knn_points, so a query's rows are distinct),
    with -1 slots, slots past the row count, and queries without a live slot (cloud 1 has no table rows, cloud 2's queries end at 211)"""
    X, Y = batch(NX, XR, 3, dtype, 7), batch(NY, SR, 3, dtype, 17)
    d2, idx = knn_points(dev(X), dev(Y), k=k, x_rows=rows_t(XR), y_rows=rows_t(SR))
    idx, d2 = idx.cpu().numpy().copy(), d2.cpu().numpy().copy()
    rng = np.random.default_rng(37)
    drop = rng.random(idx.shape) < 0.15
    idx[drop], d2[drop] = -1, np.inf
    idx[0, 5], d2[0, 5] = -1, np.inf                        # a query of a live cloud without a live slot
    idx[0, 6, :2] = SR[0] + 3                               # past the row count: not live
    F = np.where(np.isnan(Y[..., :1]), np.nan, rng.standard_normal((N, NY, C))).astype(dtype)        # NaN in the pad rows of the table
    cen = rng.standard_normal((N, NX, 3)).astype(dtype)
    return F, idx.astype(it), d2.astype(dtype), cen


def _live(idx):
    lim = torch.tensor(SR).view(-1, 1, 1)
    return (idx >= 0) & (idx < lim)


def _table_gradient_bound(F, idx, k, dtype, restate, G):
    """test_gpu_group.py's _hold_gf: the atomic table gradient within (D + k + 8) u sum|terms| of the float64 sum of its terms, D the row's
    in-degree, rows nobody names exactly 0.  The terms are linear in the cotangent with non-negative coefficients, so their float64 sum and
    the sum of their magnitudes both come from the float64 autograd of `restate` (the operator on the CPU: clamp, gather, mask)."""
    u = wl.U[np.dtype(dtype)]
    it = torch.from_numpy(idx.astype(np.int64))
    live = _live(it)
    safe = it.clamp(0, NY - 1)
    deg = torch.zeros(N, NY, dtype=torch.float64)
    deg.scatter_add_(1, safe.reshape(N, -1), live.reshape(N, -1).double())

    def grad_of(g):
        f = torch.nan_to_num(torch.from_numpy(F).double()).requires_grad_(True)
        restate(f[torch.arange(N)[:, None, None], safe], live).backward(g)
        return f.grad
    g64 = torch.from_numpy(G).double()
    ref, mag = grad_of(g64), grad_of(g64.abs())

    def check(got, outs):
        got = got.double()
        assert torch.isfinite(got).all() and (got[(deg == 0)] == 0).all()
        bound = (deg[..., None] + k + 8) * u * mag
        err = (got - ref).abs()
        assert (err <= bound).all(), float((err - bound).max())
    return check


@pytest.mark.parametrize("it", [np.int32, np.int64], ids=ids)
def test_invert_neighbors(it):
    _, idx, _, _ = _feature_case(np.float32, it)
    clean = hold(lambda: cpu(**dict(zip(("offsets", "slots"), invert_neighbors(dev(idx), NY, rows=rows_t(SR))))), label="invert_neighbors")
    assert clean["offsets"][1].max() == 0 and (clean["slots"][1] == -1).all() and clean["offsets"][0, -1] > NX


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("it", [np.int32, np.int64], ids=ids)
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
def test_group_points(det, it, dtype):
    F, idx, _, cen = _feature_case(dtype, it)
    k, C = idx.shape[2], F.shape[2]
    G = cot((N, NX, k, C), dtype, 28)

    def probe():
        f, c = dev(F).requires_grad_(True), dev(cen).requires_grad_(True)
        out = group_points(f, dev(idx), rows=rows_t(SR), centers=c, deterministic=det)
        out.backward(dev(G))
        return cpu(out=out, g_features=f.grad, g_centers=c.grad)
    atomic = {} if det else {"g_features": _table_gradient_bound(
        F, idx, k, dtype, lambda rows, live: torch.where(live[..., None], rows, torch.zeros((), dtype=torch.float64)), G)}
    clean = hold(probe, atomic=atomic, label="group_points")
    assert (clean["out"][0, 5] == 0).all() and (clean["out"][0] != 0).any() and (clean["out"][1] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("it", [np.int32, np.int64], ids=ids)
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("reduce", ["max", "mean", "sum"])
def test_pool_neighbors(reduce, det, it, dtype):
    F, idx, _, _ = _feature_case(dtype, it)
    k, C = idx.shape[2], F.shape[2]
    G = cot((N, NX, C), dtype, 29)

    def probe():
        f = dev(F).requires_grad_(True)
        res = pool_neighbors(f, dev(idx), reduce, rows=rows_t(SR), return_argmax=reduce == "max", return_counts=True, deterministic=det)
        res[0].backward(dev(G))
        return cpu(out=res[0], argmax=res[1] if reduce == "max" else None, counts=res[-1], g_features=f.grad)

    def restate(rows, live):
        z = torch.zeros((), dtype=torch.float64)
        if reduce == "max":                                 # (a query's rows are distinct and the values random: no ties)
            return torch.where(live.any(2, keepdim=True), torch.where(live[..., None], rows, z - float("inf")).amax(2), z)
        s = torch.where(live[..., None], rows, z).sum(2)
        return s if reduce == "sum" else s / live.sum(2, keepdim=True).clamp(min=1)
    atomic = {} if det else {"g_features": _table_gradient_bound(F, idx, k, dtype, restate, G)}
    clean = hold(probe, atomic=atomic, label="pool_neighbors " + reduce)
    assert clean["counts"][0, 5] == 0 and (clean["counts"][1] == 0).all() and (clean["counts"][0] > 0).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("it", [np.int32, np.int64], ids=ids)
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
def test_interpolate_features(det, it, dtype):
    """d2 >= 0 and eps > 0: d2 + eps > 0 on every live slot, so no element is one the docstring leaves unspecified"""
    F, idx, d2, _ = _feature_case(dtype, it)
    k, C = idx.shape[2], F.shape[2]
    G = cot((N, NX, C), dtype, 30)
    eps = 1e-3
    assert (d2[np.isfinite(d2)] >= 0).all()

    def probe():
        f, d = dev(F).requires_grad_(True), dev(d2).requires_grad_(True)
        out = interpolate_features(f, dev(idx), d, eps=eps, rows=rows_t(SR), deterministic=det)
        out.backward(dev(G))
        return cpu(out=out, g_features=f.grad, g_d2=d.grad)

    def restate(rows, live):
        d = torch.from_numpy(d2).double()
        live = live & torch.isfinite(d)
        r = torch.where(live, 1.0 / (torch.where(live, d, torch.ones(())) + float(dtype(eps))), torch.zeros((), dtype=torch.float64))
        w = r / r.sum(2, keepdim=True).clamp(min=1e-300)
        return (w[..., None] * torch.where(live[..., None], rows, torch.zeros((), dtype=torch.float64))).sum(2)
    atomic = {} if det else {"g_features": _table_gradient_bound(F, idx, k, dtype, restate, G)}
    clean = hold(probe, atomic=atomic, label="interpolate_features")
    assert (clean["out"][0, 5] == 0).all() and (clean["g_d2"][0] != 0).any()


# ------------------------------------------------------------------ descriptor matching

FD = 33                                                     # FPFH's width: not a multiple of the matrix-core tile's depth


def _descriptors(dtype, seed):
    """two ragged tables (N, NX, FD) / (N, NY, FD), NaN in the pad rows; the rows of fx are noisy copies of rows of fy"""
    rng = np.random.default_rng(seed)
    FY = np.full((N, NY, FD), np.nan, dtype=dtype)
    FX = np.full((N, NX, FD), np.nan, dtype=dtype)
    for b in range(N):
        FY[b, :YR[b]] = rng.standard_normal((YR[b], FD))
        src = FY[b, rng.integers(0, YR[b], XR[b])] if YR[b] else rng.standard_normal((XR[b], FD))
        FX[b, :XR[b]] = src + 0.3 * rng.standard_normal((XR[b], FD))
    return FX, FY


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
def test_knn_features(det, dtype):
    """float32: the matrix cores; float64: the vector unit"""
    k = 4
    FX, FY = _descriptors(dtype, 40)
    G = cot((N, NX, k), dtype, 41)

    def probe():
        x, y = dev(FX).requires_grad_(True), dev(FY).requires_grad_(True)
        d2, idx = knn_features(x, y, k, x_rows=rows_t(XR), y_rows=rows_t(YR), deterministic=det)
        torch.autograd.backward(d2, dev(G))
        return cpu(d2=d2, idx=idx, gfx=x.grad, gfy=y.grad)

    def check(gfy, outs):
        """test_gpu_match.py: within (L + 2) u sum|terms| of the float64 sum of the terms -2 g_is (x_i - y_j), L the row's in-degree"""
        u = wl.U[np.dtype(dtype)]
        idx, got = outs["idx"].numpy(), gfy.numpy().astype(np.float64)
        for b in range(N):
            ref, mag, deg = np.zeros((NY, FD)), np.zeros((NY, FD)), np.zeros(NY)
            live = idx[b] >= 0
            if live.any():
                i, s = np.nonzero(live)
                t = -2.0 * G[b, i, s].astype(np.float64)[:, None] * (FX[b, i].astype(np.float64) - FY[b, idx[b, i, s]].astype(np.float64))
                np.add.at(ref, idx[b, i, s], t)
                np.add.at(mag, idx[b, i, s], np.abs(t))
                np.add.at(deg, idx[b, i, s], 1.0)
            assert (got[b][deg == 0] == 0).all()
            assert (np.abs(got[b] - ref) <= (deg[:, None] + 2) * u * mag).all(), b
    clean = hold(probe, atomic={} if det else {"gfy": check}, label="knn_features")
    assert (clean["idx"][0] >= 0).all() and (clean["idx"][1:] == -1).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
def test_match_features(det, dtype):
    FX, FY = _descriptors(dtype, 42)
    G = cot((N, NX), dtype, 43)

    def probe():
        x, y = dev(FX).requires_grad_(True), dev(FY).requires_grad_(True)
        idx, d2 = match_features(x, y, x_rows=rows_t(XR), y_rows=rows_t(YR), mutual=True, ratio=0.95, max_d2=30.0, deterministic=det)
        d2.backward(torch.where(torch.isfinite(d2), dev(G), torch.zeros((), dtype=d2.dtype, device="cuda")))
        return cpu(idx=idx, d2=d2, gfx=x.grad, gfy=y.grad)
    # mutual matches name every row of fy at most once: the y-gradient's sums have a single term, exact under both backward forms
    clean = hold(probe, label="match_features")
    assert (clean["idx"][0] >= 0).any() and (clean["idx"][0] < 0).any() and (clean["idx"][1:] == -1).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_soft_match_features(dtype):
    FX, FY = _descriptors(dtype, 44)
    V = batch(NY, YR, 6, dtype, 45)
    G = cot((N, NX, 6), dtype, 46)

    def probe():
        x, y, v = dev(FX).requires_grad_(True), dev(FY).requires_grad_(True), dev(V).requires_grad_(True)
        out, idx, prob = soft_match_features(x, y, v, 4.0, x_rows=rows_t(XR), y_rows=rows_t(YR), return_best=True)
        out.backward(dev(G))
        return cpu(out=out, idx=idx, prob=prob, gfx=x.grad, gfy=y.grad, gvalues=v.grad)
    clean = hold(probe, label="soft_match_features")
    assert (clean["idx"][0] >= 0).all() and (clean["out"][1:] == 0).all() and (clean["gvalues"][0] != 0).any()


# ------------------------------------------------------------------ correspondences: fits, residuals, compatibility, consensus

PR = (300, 0, 211)


@functools.lru_cache(maxsize=None)
def _pairs(dtype, clean):
    """compat_cases.cloud per cloud of the batch: clean -- every row below the count a live pair, idx an injection (each row of y named at
    most once), 60 % inliers; otherwise its dead rows of every kind below the count (idx < 0, a NaN in x, an inf in the matched row of y) and a
    clamped index, 30 % inliers.  Cloud 1 has 0 rows."""
    X, Y, I = np.zeros((N, NX, 3), dtype), np.zeros((N, NY, 3), dtype), np.zeros((N, NX), np.int64)
    for b, r in enumerate(PR):
        rng = np.random.default_rng(60 + b)
        X[b], Y[b], I[b] = cc.cloud(rng, NX, NY, r if clean else (2 * r) // 3, dtype, rows=r, inlier_ratio=0.6 if clean else 0.3, clamp=not clean)
        if clean:
            I[b, r:] = -1
    W = (np.random.default_rng(59).random((N, NX)) + 0.5).astype(dtype)
    return X, Y, I, W


def _fit_probe(fit, dtype, weighted=True):
    X, Y, I, W = _pairs(dtype, True)
    GT = cot((N, 4, 4), dtype, 61)

    def probe():
        x, y = dev(X).requires_grad_(True), dev(Y).requires_grad_(True)
        w = dev(W).requires_grad_(True) if weighted else None
        outs = fit(x, y, dev(I), w, rows_t(PR))
        T = outs["T"]
        # cloud 1 has no pair: "the gradients at such a point are not meaningful" (align_correspondences) -- its pose, which is compared like
        # every other, takes no cotangent, so that the gradients of all three clouds stay defined
        T[[0, 2]].backward(dev(GT)[[0, 2]])
        return cpu(gx=x.grad, gy=y.grad, gw=w.grad if weighted else None, **outs)
    return probe


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "unit"])
def test_align_correspondences(weighted, dtype):
    """idx is injective: gy's sums have a single term each, so every gradient is exact"""
    probe = _fit_probe(lambda x, y, i, w, r: dict(T=align_correspondences(x, y, i, weight=w, x_rows=r)), dtype, weighted)
    clean = hold(probe, label="align_correspondences")
    assert torch.isfinite(clean["T"][[0, 2]]).all() and (clean["gy"][0] != 0).any() and (clean["gx"][1] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_ransac_correspondences(dtype):
    def fit(x, y, i, w, r):
        T, inl, best, count, Tb = ransac_correspondences(x, y, i, 0.05, hypotheses=64, seed=5, refine=2, weight=w, x_rows=r, return_hypothesis=True)
        return dict(T=T, inliers=inl, best=best, best_count=count, T_best=Tb)
    clean = hold(_fit_probe(fit, dtype), label="ransac_correspondences")
    assert clean["best"].tolist()[1] == -1 and clean["inliers"][0].sum() > 100 and not clean["inliers"][1].any()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("loss", ["tls", "gm"])
def test_gnc_correspondences(loss, dtype):
    def fit(x, y, i, w, r):
        T, wg, rounds, status, mu, Tl = gnc_correspondences(x, y, i, 0.05, loss=loss, weight=w, x_rows=r, return_info=True)
        return dict(T=T, weights=wg, rounds=rounds, status=status, mu=mu, T_last=Tl)
    clean = hold(_fit_probe(fit, dtype), label="gnc_correspondences " + loss)
    assert clean["status"].tolist()[1] == 3 and clean["rounds"][0] > 0 and (clean["weights"][0] > 0).sum() > 100


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_consensus_correspondences(dtype):
    def fit(x, y, i, w, r):
        T, inl, best, count, Tb, mem = consensus_correspondences(x, y, i, 0.05, seeds=32, members=8, refine=1, weight=w, x_rows=r, return_hypothesis=True)
        return dict(T=T, inliers=inl, best=best, best_count=count, T_best=Tb, members=mem)
    clean = hold(_fit_probe(fit, dtype), label="consensus_correspondences")
    assert clean["best"].tolist()[1] == -1 and clean["inliers"][0].sum() > 100


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("op", ["residuals", "compatibility", "second_order", "prune 1", "prune 2"])
def test_correspondence_decisions(op, dtype):
    """on compat_cases.cloud with its dead rows of every kind: each is "not live" by rule 1, a defined result"""
    X, Y, I, _ = _pairs(dtype, False)
    T = np.tile(np.eye(4, dtype=dtype), (N, 1, 1))
    T[:, :3, 3] = 0.01

    def probe():
        x, y, i, r = dev(X), dev(Y), dev(I), rows_t(PR)
        if op == "residuals":
            return cpu(d2=correspondence_residuals(x, y, i, dev(T), x_rows=r))
        if op == "compatibility":
            return cpu(**dict(zip(("score", "degree"), correspondence_compatibility(x, y, i, cc.TAU, iterations=4, min_length=0.1, x_rows=r))))
        if op == "second_order":
            return cpu(**dict(zip(("score2", "degree2", "degree", "adjacency"),
                                  second_order_compatibility(x, y, i, cc.TAU, min_length=0.1, x_rows=r, return_adjacency=True))))
        return cpu(**dict(zip(("idx_kept", "score"), prune_correspondences(x, y, i, cc.TAU, 40, iterations=4, x_rows=r, order=int(op[-1])))))
    clean = hold(probe, label=op)
    first = clean[sorted(clean)[0]]
    assert (first[0] != first[0, 0]).any()


# ------------------------------------------------------------------ FPFH, ISS

K_NB = 12


def _with_empty_slots(idx, rows, seed):
    """-1, -7 and rows at and past the count in 8 % of the slots (the generators' own garbage, without their non-finite rows below the count)"""
    rng = np.random.default_rng(seed)
    hit = rng.random(idx.shape) < 0.08
    idx[hit] = rng.choice(np.array([-1, -7, rows, rows + 1], dtype=np.int64), int(hit.sum()))
    return idx


@functools.lru_cache(maxsize=None)
def _fpfh_batch(dtype):
    clouds = [fc.random_cloud(70 + b, NY, K_NB, dtype, rows=r, cols=6, garbage=False) for b, r in enumerate(SR)]
    for c in clouds:
        _with_empty_slots(c["idx"], c["rows"], 75)
    return fc.pad_batch(clouds, m=NY, k=K_NB)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("it", [np.int32, np.int64], ids=ids)
def test_fpfh_features(it, dtype):
    P, Nn, idx, rows = _fpfh_batch(dtype)
    clean = hold(lambda: cpu(**dict(zip(("out", "spfh"), fpfh_features(dev(P), dev(Nn), dev(idx.astype(it)), rows=rows_t(SR), radius=0.6, return_spfh=True)))),
                 label="fpfh_features")
    assert (clean["out"][0] != 0).any() and (clean["out"][1] == 0).all() and (clean["spfh"][0] != 0).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_compute_fpfh(dtype):
    P, Nn, _, _ = _fpfh_batch(dtype)
    clean = hold(lambda: cpu(out=compute_fpfh(dev(P[..., :3].copy()), dev(Nn), 0.6, k=K_NB, rows=rows_t(SR))), label="compute_fpfh")
    assert (clean["out"][0] != 0).any() and (clean["out"][1] == 0).all()


@functools.lru_cache(maxsize=None)
def _iss_batch(dtype):
    clouds = [ic.random_cloud(80 + b, NY, K_NB, dtype, rows=r, cols=6, garbage=False) for b, r in enumerate(SR)]
    for c in clouds:
        _with_empty_slots(c["idx"], c["rows"], 85)
    radius = ic.median_radius(clouds[0], 0.8)
    P, idx, _ = ic.pad_batch(clouds, m=NY, k=K_NB)
    return P, idx, radius


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("it", [np.int32, np.int64], ids=ids)
def test_iss_on_neighbour_lists(it, dtype):
    P, idx, radius = _iss_batch(dtype)

    def probe():
        x, i, r = dev(P), dev(idx.astype(it)), rows_t(SR)
        sal, eig, cnt = iss_saliency(x, i, rows=r, radius=radius, min_neighbors=4, return_eigenvalues=True, return_counts=True)
        mask, sal2 = iss_keypoints(x, i, rows=r, salient_radius=radius, non_max_radius=radius, min_neighbors=4, return_saliency=True)
        return cpu(saliency=sal, eigenvalues=eig, counts=cnt, mask=mask, saliency_of_keypoints=sal2)
    clean = hold(probe, label="iss_saliency, iss_keypoints")
    assert clean["mask"][0].any() and not clean["mask"][1].any() and (clean["counts"][0] > 4).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_iss_whole_ball(dtype):
    P, _, _ = _iss_batch(dtype)
    r1 = 0.3

    def probe():
        x, r = dev(P), rows_t(SR)
        sal, eig, cnt = iss_saliency_ball(x, r1, rows=r, min_neighbors=4, return_eigenvalues=True, return_counts=True)
        mask, sal2 = iss_keypoints_ball(x, r1, 0.25, rows=r, min_neighbors=4, return_saliency=True)
        return cpu(saliency=sal, eigenvalues=eig, counts=cnt, mask=mask, saliency_of_keypoints=sal2)
    clean = hold(probe, label="iss_saliency_ball, iss_keypoints_ball")
    assert clean["mask"][0].any() and not clean["mask"][1].any()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("whole_ball", [False, True], ids=["lists", "ball"])
def test_compute_iss_keypoints(whole_ball, dtype):
    P, _, _ = _iss_batch(dtype)
    Pf = np.where(np.isnan(P[..., 3:]) & ~np.isnan(P[..., :1]), np.float64(0.5), P[..., 3:])      # finite extra columns below the count: they are carried along
    Pc = np.concatenate((P[..., :3], Pf), 2).astype(dtype)

    def probe():
        x = dev(Pc).requires_grad_(True)
        kp, rows_out, index = compute_iss_keypoints(x, 0.3, 0.25, k=K_NB, rows=rows_t(SR), min_neighbors=4, return_index=True, whole_ball=whole_ball)
        kp.backward(dev(cot(tuple(kp.shape), dtype, 86)))
        return cpu(keypoints=kp, rows_out=rows_out, index=index, grad=x.grad)
    clean = hold(probe, label="compute_iss_keypoints")
    assert clean["rows_out"][0] > 0 and clean["rows_out"][1] == 0


# ------------------------------------------------------------------ evaluate_registration, information_matrix


def _poses(H, dtype, seed):
    rng = np.random.default_rng(seed)
    T = np.tile(np.eye(4), (N, H, 1, 1))
    T[..., :3, 3] = 0.02 * rng.standard_normal((N, H, 3))
    a = 0.02 * rng.standard_normal((N, H))
    T[..., 0, 0], T[..., 0, 1], T[..., 1, 0], T[..., 1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    return T.astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("H", [1, 5])
def test_evaluate_registration(H, dtype):
    X, Y, T = batch(NX, XR, 6, dtype, 90), batch(NY, (330, 170, 200), 6, dtype, 90), _poses(H, dtype, 91)
    yr = (330, 170, 200)

    def probe():
        fit, rmse, counts, idx, d2 = evaluate_registration(dev(X), dev(Y), dev(T), 0.08, rows_t(XR), rows_t(yr), return_correspondences=True)
        return cpu(fitness=fit, rmse=rmse, counts=counts, idx=idx, d2=d2)
    clean = hold(probe, label="evaluate_registration H=%d" % H)
    assert (clean["counts"][0] > 0).all() and (clean["counts"][1] == 0).all() and (clean["idx"][0] < 0).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_information_matrix(dtype):
    X, Y, T = batch(NX, XR, 6, dtype, 90), batch(NY, YR, 6, dtype, 90), _poses(1, dtype, 92)[:, 0]
    clean = hold(lambda: cpu(information=information_matrix(dev(X), dev(Y), dev(T), 0.08, rows_t(XR), rows_t(YR))), label="information_matrix")
    assert (clean["information"][0] != 0).any() and (clean["information"][1:] == 0).all()


# ------------------------------------------------------------------ the ICP loop: one probe per buffer plan of _loop.py / _call.py

FIRST, SECOND = (0, 1, 3), (2, 4, 6)            # clouds of icp_rows_ref.batch(): 320/257/129 source rows with 400/129/257 target rows, then 256/128/64 with 385/128/400
K_ICP = 5
FORWARD = ("T", "pc", "deltas", "costs", "weights", "converged", "iterations", "matched_ratio")
# (case of tests/icp_rows_ref.py, attributes of the ICP object, dicp_amd._loop.CERT_MIN_WORK: 0 = certificates at every size, the suite's default)
ICP_PLANS = {
    "brute force, atomic backward, weight": (R.case(weight="point", thresh=0.3, K=K_ICP), dict(knn_variant=_lib.KNN_VALU), 0.0),
    "sweep, windowed pt2pt (c = cv), tolerance mode": (R.case(icp_type="pt2pt", mode="tol", K=K_ICP), dict(knn_variant=_lib.KNN_SWEEP, bwd_window=True), 0.0),
    # (certificates need three certified iterations: with 5 iterations the certifying search has to be iteration 1 -- the short re-order schedule)
    "sweep, windowed pt2pl (c != cv), weight, certificates": (R.case(weight="point", thresh=0.3, K=K_ICP), dict(knn_variant=_lib.KNN_SWEEP, bwd_window=True, reuse_matches=True,
                                                                                                                 _tuning=dict(sweep_resort=(0, 1))), 0.0),
    "sweep, windowed pt2pl, plain searches": (R.case(K=K_ICP), dict(knn_variant=_lib.KNN_SWEEP, bwd_window=True), 2.0e6),
    "sweep, windowed pt2pl, tolerance mode, cloud weight": (R.case(mode="tol", weight="cloud", K=K_ICP), dict(knn_variant=_lib.KNN_SWEEP, bwd_window=True), 0.0),
    "sweep, atomic backward": (R.case(K=K_ICP), dict(knn_variant=_lib.KNN_SWEEP, bwd_window=False), 0.0),
    "deterministic": (R.case(weight="point", thresh=0.3, K=K_ICP), dict(deterministic=True), 0.0),
}


@functools.lru_cache(maxsize=None)
def _cloud_reference(c, b):
    return R.run_cloud(c, b)


def _rows_call(icp, c, clouds, tag):
    """one call on clouds `clouds` of icp_rows_ref.batch() as a padded batch with row counts, loss sum(T gT) + sum over own rows of pc gpc"""
    d, sel = R.batch(), list(clouds)
    cols = 6 if c.icp_type == "pt2pl" else 3
    put = lambda x: x[sel].clone().cuda().contiguous().requires_grad_(True)       # noqa: E731
    src, tgt, T0 = put(d["source"]), put(d["target"][:, :, :cols]), put(d["T_init"])
    w = None if c.weight == "none" else put(R.weight_of(c))
    ls, lt = [R.LS[b] for b in sel], [R.LT[b] for b in sel]
    out = icp.icp(src, tgt, T0, weight=w, trim_dist=c.trim, loss_fn=R.LOSSES[c.loss], dim=c.dim, source_rows=rows_t(ls), target_rows=rows_t(lt))
    gT, gpc = d["gT"][sel].cuda(), d["gpc"][sel].cuda()
    loss = (out["T"] * gT).sum()
    for i, n in enumerate(ls):
        loss = loss + (out["pc"][i, :n] * gpc[i, :n]).sum()
    loss.backward()
    named = dict(g_source=src.grad, g_target=tgt.grad, g_T_init=T0.grad, g_weight=None if w is None else w.grad, **{k: out[k] for k in FORWARD[:5]}, **out["stats"])
    return {tag + k: v for k, v in cpu(**named).items()}


def _held_to_the_oracle(c, clouds, tag, key):
    """tests/test_gpu_icp_rows.py's float64 bars (those of tests/test_gpu_parity.py): a gradient within 1e-9 + 1e-8 |reference| of the per-cloud
    float64 oracle on the cloud's own rows, exactly 0 on the pads"""
    def check(got, outs):
        got = got.numpy()
        for i, b in enumerate(clouds):
            want = _cloud_reference(c, b)["grad_" + key]
            rows = {"source": R.LS[b], "target": R.LT[b], "T_init": 4, "weight": R.LS[b] if c.weight == "point" else 1}[key]
            np.testing.assert_allclose(got[i, :rows], want.numpy(), rtol=1e-8, atol=1e-9, err_msg="%sgrad %s of cloud %d" % (tag, key, b))
            if key != "T_init" and not (key == "weight" and c.weight == "cloud"):
                assert (got[i, rows:] == 0).all(), (tag, key, b, "gradient on the pads")
    return check


@pytest.mark.parametrize("plan", list(ICP_PLANS))
def test_icp_loop_on_a_ragged_batch(plan, monkeypatch):
    """float64, 3 clouds of 129 .. 320 rows against 129 .. 400, 5 iterations, forward + backward to source, target, weight and T_init, and the same
    ICP object a second time on other clouds of the same shape (_bwd_truncation_and_tail and the hints use the earlier calls' counters).  The
    forward is exact; so is every gradient with ICP.deterministic.  Otherwise a target row's contributions are summed in the order the waves
    reach it and the backward's slot order is not reproducible inside a bucket (ICP.deterministic's comment): the gradients are held to the
    float64 oracle."""
    c, attrs, cert_min_work = ICP_PLANS[plan]
    monkeypatch.setattr(_loop, "CERT_MIN_WORK", cert_min_work)
    certified = []

    def probe():
        icp = ICP(icp_type=c.icp_type, differentiable=c.diff, max_iterations=c.K, tolerance=c.tol)
        icp.const_iter, icp.match_ratio_thresh = (c.mode == "const"), c.thresh
        for k, v in attrs.items():
            icp._tuning.update(v) if k == "_tuning" else setattr(icp, k, v)
        outs = _rows_call(icp, c, FIRST, "1 ")
        outs.update(_rows_call(icp, c, SECOND, "2 "))
        certified.append("searched_again" in icp.knn_stats)
        return outs
    grads = ["source", "target", "T_init"] + ([] if c.weight == "none" else ["weight"])
    atomic = {} if plan == "deterministic" else {tag + "g_" + key: _held_to_the_oracle(c, clouds, tag, key)
                                                 for tag, clouds in (("1 ", FIRST), ("2 ", SECOND)) for key in grads}
    clean = hold(probe, atomic=atomic, monkeypatch=monkeypatch, label="ICP " + plan)
    if "certificates" in plan or "plain searches" in plan:  # the plan its name promises: the certificates' arrays are allocated, or not
        assert certified == [plan.endswith("certificates")] * 3, certified
    for tag, clouds in (("1 ", FIRST), ("2 ", SECOND)):     # the clean forward is the oracle's (the bars of tests/test_gpu_icp_rows.py)
        for i, b in enumerate(clouds):
            np.testing.assert_allclose(clean[tag + "T"][i].numpy(), _cloud_reference(c, b)["T"].numpy(), rtol=0, atol=1e-10)
        assert (clean[tag + "g_target"] != 0).any()


def _dense_case(N, n, m, K, seed):
    src, tgt = make_pairs(N, n, m, seed=seed, dtype=torch.float64, max_rot=0.03, max_trans=0.1)
    gen = torch.Generator().manual_seed(seed + 1)
    rnd = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64)       # noqa: E731
    T0 = torch.eye(4, dtype=torch.float64).repeat(N, 1, 1)
    T0[:, :3, 3] = 0.02 * rnd(N, 3)
    return dict(src=src, tgt=tgt, T0=T0, gT=rnd(N, 4, 4), gpc=rnd(N, n, 3), w=0.5 + torch.rand((N, n), generator=gen, dtype=torch.float64))


KW = dict(trim_dist=5.0, loss_fn={"name": "huber", "metric": 1.0}, dim=3)


def _dense_oracle(d, K, weighted, **kw):
    s, t, T0 = (d[k].clone().requires_grad_(True) for k in ("src", "tgt", "T0"))
    w = d["w"].clone().requires_grad_(True) if weighted else None
    ref = O.icp_batched(s, t, T0, torch.ones_like(d["w"]) if w is None else w, icp_type="pt2pl", differentiable=True, max_iterations=K, tolerance=1e-14,
                        const_iter=True, tanh_steepness=5.0, **KW, **kw)
    ((ref["T"] * d["gT"]).sum() + (ref["pc"] * d["gpc"]).sum()).backward()
    return dict(T=ref["T"].detach(), g_source=s.grad, g_target=t.grad, g_T_init=T0.grad, g_weight=None if w is None else w.grad)


def _dense_call(icp, d, weighted):
    s, t, T0 = (d[k].clone().cuda().requires_grad_(True) for k in ("src", "tgt", "T0"))
    w = d["w"].clone().cuda().requires_grad_(True) if weighted else None
    out = icp.icp(s, t, T0, weight=w, **KW)
    ((out["T"] * d["gT"].cuda()).sum() + (out["pc"] * d["gpc"].cuda()).sum()).backward()
    return cpu(g_source=s.grad, g_target=t.grad, g_T_init=T0.grad, g_weight=None if w is None else w.grad, **{k: out[k] for k in FORWARD[:5]}, **out["stats"])


def _dense_bars(ref, key):
    """smoke()'s and tests/test_gpu_gumbel.py's bar on gradients against the float64 oracle: 1e-8"""
    def check(got, outs):
        assert float((got - ref[key]).abs().max()) < 1e-8, key
    return check


@pytest.mark.parametrize("weighted", [False, True], ids=["weight None", "weight"])
def test_icp_one_call_path(weighted, monkeypatch):
    """dicp_call_forward / _backward on one allocation (_call.CallLoop): a dense batch, constant iterations, the sweep search, no certificates"""
    N, n, m, K = 3, 500, 600, 4
    monkeypatch.setattr(_loop, "CERT_MIN_WORK", 2.0e6)
    d = _dense_case(N, n, m, K, 11)
    ref = _dense_oracle(d, K, weighted)
    taken = []
    real = _call.CallLoop.apply
    monkeypatch.setattr(_call.CallLoop, "apply", staticmethod(lambda *a: (taken.append(1), real(*a))[1]))

    def probe():
        icp = ICP(icp_type="pt2pl", differentiable=True, max_iterations=K, tolerance=1e-14)
        icp.const_iter, icp.knn_variant = True, _lib.KNN_SWEEP
        return _dense_call(icp, d, weighted)
    grads = ["g_source", "g_target", "g_T_init"] + (["g_weight"] if weighted else [])
    clean = hold(probe, atomic={k: _dense_bars(ref, k) for k in grads}, monkeypatch=monkeypatch, label="ICP one-call path")
    assert len(taken) == 3 and float((clean["T"] - ref["T"]).abs().max()) < 1e-9


def test_icp_gumbel_soft_correspondences(monkeypatch):
    """the soft loop with its draws pinned (nn._inject_U, as tests/test_gpu_gumbel.py pins them); the oracle reads the same draws through torch.rand"""
    N, n, m, K = 3, 300, 600, 2
    d = _dense_case(N, n, m, K, 63)
    Us = [torch.tensor(G.hash_uniform(50 + k, N, n, m)) for k in range(K)]
    draws = iter(Us)
    with monkeypatch.context() as mp:
        mp.setattr(torch, "rand", lambda *a, **k: next(draws))
        ref = _dense_oracle(d, K, False, use_gumbel=True, gumbel_eps=1e-10, gumbel_tau=0.1)

    def probe():
        icp = ICP(icp_type="pt2pl", differentiable=True, max_iterations=K, tolerance=1e-14)
        icp.const_iter = True
        icp.nn.use_gumbel, icp.nn.eps, icp.nn.tau = True, 1e-10, 0.1
        icp.nn._inject_U = [u.cuda() for u in Us]
        return _dense_call(icp, d, False)
    clean = hold(probe, atomic={k: _dense_bars(ref, k) for k in ("g_source", "g_target", "g_T_init")}, monkeypatch=monkeypatch, label="ICP Gumbel")
    assert float((clean["T"] - ref["T"]).abs().max()) < 1e-9


def test_icp_f16_sweep(monkeypatch):
    """float32, the matrix-core sweep switched on as tests/test_gpu_f16.py switches it on (that size: the form is taken from 16384 targets on).  The
    forward is exact; the gradients are held, with that test's bar of 1e-5 of the largest entry, to the same call on the vector unit."""
    N, n, K = 2, 32768, 3
    src, tgt = make_pairs(N, n, n, seed=21)
    gen = torch.Generator().manual_seed(22)
    gT, gpc = torch.randn((N, 4, 4), generator=gen), torch.randn((N, n, 3), generator=gen)
    monkeypatch.setattr(_ops, "F16_SWEEP_MIN_QUERIES", 0)

    def probe():
        icp = ICP(icp_type="pt2pl", differentiable=True, max_iterations=K, tolerance=1e-12)
        icp.const_iter, icp.knn_variant = True, _lib.KNN_SWEEP | (2 << 8)
        s, t = src.cuda().requires_grad_(True), tgt.cuda().requires_grad_(True)
        out = icp.icp(s, t, torch.eye(4, device="cuda").repeat(N, 1, 1), **KW)
        ((out["T"] * gT.cuda()).sum() + (out["pc"] * gpc.cuda()).sum()).backward()
        return cpu(g_source=s.grad, g_target=t.grad, **{k: out[k] for k in FORWARD[:5]}, **out["stats"])
    monkeypatch.setattr(_ops, "F16_SWEEP", False)
    ref = probe()
    monkeypatch.setattr(_ops, "F16_SWEEP", True)

    def bar(key):
        def check(got, outs):
            assert torch.equal(outs["T"], ref["T"]) and torch.equal(outs["deltas"], ref["deltas"])
            assert float((got - ref[key]).abs().max()) <= 1e-5 * float(ref[key].abs().max()), key
        return check
    hold(probe, atomic={k: bar(k) for k in ("g_source", "g_target")}, monkeypatch=monkeypatch, label="ICP f16 sweep")


@pytest.mark.parametrize("weighted", [False, True], ids=["weight None", "weight"])
def test_pt2pt_dICP_SVD_one_call(weighted, monkeypatch):
    """ICP.pt2pt_dICP_SVD through _call.KabschCall, held as tests/test_gpu_call.py holds it: the gradients within 1e-12 of the largest entry of
    KabschLoop's (the per-buffer loop; its target gradient is row atomics), the forward exact"""
    N, n, m, K = 3, 500, 600, 4
    d = _dense_case(N, n, m, K, 31)

    def probe(one=True):
        icp = ICP(icp_type="pt2pt", differentiable=True, max_iterations=K, tolerance=1e-12)
        icp.const_iter, icp.knn_variant = True, _lib.KNN_SWEEP
        icp._tuning["one_call"] = one
        s, t = d["src"].clone().cuda().requires_grad_(True), d["tgt"].clone().cuda().requires_grad_(True)
        w = d["w"].clone().cuda().requires_grad_(True) if weighted else None
        pc, T = icp.pt2pt_dICP_SVD(s, t, d["T0"].cuda(), trim_dist=3.0, weight=w)
        ((T * d["gT"].cuda()).sum() + (pc * d["gpc"].cuda()).sum()).backward()
        return cpu(pc=pc, T=T, costs=icp.svd_stats["costs"], iterations=icp.svd_stats["iterations"], g_source=s.grad, g_target=t.grad,
                   g_weight=None if w is None else w.grad)
    ref = probe(one=False)

    def bar(key):
        def check(got, outs):
            assert float((got - ref[key]).abs().max()) <= 1e-12 * max(1e-30, float(ref[key].abs().max())), key
        return check
    taken = []
    real = _call.KabschCall.apply
    monkeypatch.setattr(_call.KabschCall, "apply", staticmethod(lambda *a: (taken.append(1), real(*a))[1]))
    hold(probe, atomic={k: bar(k) for k in ["g_source", "g_target"] + (["g_weight"] if weighted else [])}, monkeypatch=monkeypatch, label="pt2pt_dICP_SVD")
    assert len(taken) == 3
