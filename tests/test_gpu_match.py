"""Descriptor matching on the MI355X: knn_features, match_features, align_correspondences (dicp_amd/match.py).

1  the forward index for index and bit for bit against the numpy restatement tests/match_ref.py -- float64, and float32 in both forms
   (matrix cores and vector unit) and the two forms against each other -- around the 32-row tile, the LDS stage, odd D, one channel pair
   and the cap, with k > m, ragged rows (0 included), list and single forms and pad rows holding NaN and 1e30;
2  designed inputs: duplicates across a tile edge and across a query's two lanes, a query equal to a row, score ties with different d2,
   non-finite rows on both sides, an overflowing h, subnormals, norms 1 and 1e3;
3  the chain property of the matrix-core instruction where it can go wrong: D = 256 with heavy cancellation;
4  against the truth (float64 distances) within the derived forward-error bounds of the two chains;
5  the gradients within (L + 2) u sum|terms| of float64 autograd, deterministic=True bit for bit against the restatement's order;
6  match_features rule by rule against the restatement;  7  align_correspondences against a float64 numpy SVD Kabsch and autograd through
   torch.linalg.svd;  8  descriptors -> match -> align -> ICP end to end;  9  knn_features forward + backward in a captured graph.
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.ICP import ICP
from dicp_amd.match import align_correspondences, knn_features, match_features

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_cases as mc  # noqa: E402
import match_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu

TD = {np.float32: torch.float32, np.float64: torch.float64}
UNIT = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    """a float tensor as integers (NaN in the same places compares equal only with the same payload: the outputs hold none)"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and (torch.equal(bits(a), bits(b)) if a.dtype.is_floating_point else torch.equal(a, b))


def descr(rng, n, m, D, dtype):
    y = rng.standard_normal((m, D)).astype(dtype)
    x = (y[rng.integers(0, m, n)] + 0.3 * rng.standard_normal((n, D))).astype(dtype)
    return x, y


def forms(dtype):
    return (None, "valu", "mfma") if dtype == np.float32 else (None,)


def check_against_ref(x, y, k, dtype, x_rows=None, y_rows=None):
    """every form on the batch x (N, n, D), y (N, m, D) -> the restatement's d2, idx per cloud"""
    N = x.shape[0]
    ref = [mr.knn_features_ref(x[b], y[b], k, None if x_rows is None else x_rows[b], None if y_rows is None else y_rows[b]) for b in range(N)]
    rd2, ridx = dev(np.stack([r[0] for r in ref])), dev(np.stack([r[1] for r in ref]))
    rx = None if x_rows is None else torch.tensor(x_rows, dtype=torch.int32).cuda()
    ry = None if y_rows is None else torch.tensor(y_rows, dtype=torch.int64).cuda()
    for form in forms(dtype):
        d2, idx = knn_features(dev(x), dev(y), k, x_rows=rx, y_rows=ry, _form=form)
        assert idx.dtype == torch.int64 and d2.dtype == TD[dtype]
        assert torch.equal(idx, ridx), form
        assert same(d2, rd2), form
    return ref


# ------------------------------------------------------------------ 1
F32_CASES = [(1, 1, 1, 1), (31, 2, 2, 2), (33, 2, 31, 5), (32, 31, 3, 4), (33, 32, 31, 5), (65, 33, 32, 8), (300, 63, 33, 16), (33, 64, 64, 17),
             (32, 65, 255, 32), (31, 300, 256, 8), (65, 1100, 32, 4), (300, 300, 3, 32), (1, 1100, 2, 1), (65, 65, 1, 2)]
F64_CASES = [(1, 1, 1, 1), (31, 2, 3, 2), (33, 33, 2, 5), (3, 65, 33, 17), (2, 32, 256, 4), (5, 300, 3, 32), (33, 31, 31, 8), (4, 64, 64, 16)]


@pytest.mark.parametrize("case", [(np.float32,) + c for c in F32_CASES] + [(np.float64,) + c for c in F64_CASES])
def test_forward_is_the_restatement(case):
    dtype, n, m, D, k = case
    rng = np.random.default_rng(n + 7 * m + 13 * D + k)
    x = np.stack([descr(rng, n, m, D, dtype)[0] for _ in range(3)])
    y = np.stack([descr(rng, n, m, D, dtype)[1] for _ in range(3)])
    x_rows, y_rows = [n, n // 2, n], [m, max(m - 1, 0), 0]
    x[1, x_rows[1]:] = np.nan
    y[1, y_rows[1]:] = np.nan                               # pad rows: kept out by the row count, whatever they hold
    y[2] = 1e30
    ref = check_against_ref(x, y, k, dtype, x_rows, y_rows)
    assert (ref[0][1][:, :min(k, m)] >= 0).all() and (ref[0][1][:, min(k, m):] == -1).all()      # k > m: the tail is empty
    assert (ref[2][1] == -1).all() and (ref[1][1][x_rows[1]:] == -1).all()
    # single clouds and lists give the batch's clouds
    d2s, idxs = knn_features(dev(x[0]), dev(y[0]), k)
    assert torch.equal(idxs, dev(ref[0][1])) and same(d2s, dev(ref[0][0]))
    xl, yl = [dev(x[b, :x_rows[b]]) for b in range(2)], [dev(y[b, :y_rows[b]]) for b in range(2)]
    d2l, idxl = knn_features(xl, yl, k)
    for b in range(2):
        assert torch.equal(idxl[b], dev(ref[b][1][:x_rows[b]])) and same(d2l[b], dev(ref[b][0][:x_rows[b]]))


def test_cpu_tensors_and_empty_clouds():
    rng = np.random.default_rng(21)
    x, y = descr(rng, 9, 14, 5, np.float32)
    rd2, ridx = mr.knn_features_ref(x, y, 3)
    d2, idx = knn_features(torch.from_numpy(x), torch.from_numpy(y), 3)                # CPU tensors: computed on the GPU, returned on the CPU
    assert not d2.is_cuda and not idx.is_cuda and torch.equal(idx, torch.from_numpy(ridx)) and same(d2, torch.from_numpy(rd2))
    mi, md = match_features(torch.from_numpy(x), torch.from_numpy(y), mutual=True)
    ri, rd = mr.match_features_ref(x, y, mutual=True)
    assert not mi.is_cuda and torch.equal(mi, torch.from_numpy(ri)) and same(md, torch.from_numpy(rd))
    d2, idx = knn_features(dev(x), dev(y[:0]), 2)                                       # no rows to search: every slot empty
    assert d2.shape == (9, 2) and (idx == -1).all() and torch.isinf(d2).all()
    d2, idx = knn_features(dev(x[:0]), dev(y), 2)
    assert d2.shape == (0, 2) and idx.shape == (0, 2)


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_designed_inputs(dtype):
    rng = np.random.default_rng(11)
    n, m, D, k = 40, 100, 8, 8
    x, y = descr(rng, n, m, D, dtype)
    dup = [3, 4, 31, 32, 70]                                # rows 3 | 4: the two lanes of a query; 31 | 32: a tile edge
    y[dup] = y[3]
    x[0] = y[3]                                             # a query equal to a row
    y[10, 2] = np.nan; y[11, 0] = np.inf; y[12, D - 1] = -np.inf      # never returned
    x[5, 1] = np.nan; x[6, 7] = np.inf                      # no neighbours
    big = np.finfo(dtype).max
    y[13] = big / 2                                         # h overflows to +inf: excluded
    tiny = np.finfo(dtype).tiny
    y[14] = tiny / 4; y[15] = tiny / 8; x[7] = tiny / 16     # subnormal channels
    ref = check_against_ref(x[None], y[None], k, dtype)[0]
    d2, idx = ref
    assert list(idx[0, :5]) == dup and np.all(d2[0, :5] == 0) and not np.signbit(d2[0, :5]).any()
    assert not np.isin(idx, (10, 11, 12, 13)).any()
    assert np.all(idx[5] == -1) and np.all(idx[6] == -1) and np.all(np.isinf(d2[5]))
    assert np.isin(idx[7, :2], (14, 15)).all()
    for kk in (1, 2):                                       # the lowest index wins; all duplicates in index order
        assert list(check_against_ref(x[None, :1], y[None], kk, dtype)[0][1][0]) == dup[:kk]
    for scale in (1.0, 1e3):                                # descriptors of norm 1 and of norm 1e3
        xs, ys = descr(rng, 33, 130, 32, dtype)
        xs = (scale * xs / np.linalg.norm(xs, axis=1, keepdims=True)).astype(dtype)
        ys = (scale * ys / np.linalg.norm(ys, axis=1, keepdims=True)).astype(dtype)
        check_against_ref(xs[None], ys[None], 4, dtype)


def test_scores_that_tie_while_d2_differs():
    rng = np.random.default_rng(12)
    base = (5.0 * rng.standard_normal((1, 16))).astype(np.float32)
    y = (base + 1e-6 * rng.standard_normal((96, 16))).astype(np.float32)      # near-duplicates: the score's ulp is far above the d2's
    x = (base + 1e-6 * rng.standard_normal((33, 16))).astype(np.float32)
    d2, idx, sc = mr.knn_features_ref(x, y, 8, return_scores=True)
    tie = (sc[:, 1:] == sc[:, :-1]) & (d2[:, 1:] != d2[:, :-1])
    assert tie.any() and (idx[:, 1:][tie] > idx[:, :-1][tie]).all()           # the input has such ties; the index decides them
    check_against_ref(x[None], y[None], 8, np.float32)


# ------------------------------------------------------------------ 3
def test_chain_property_under_cancellation():
    rng = np.random.default_rng(13)
    n, m, D = 64, 96, 256
    y = (rng.standard_normal((m, D)) * np.exp(rng.uniform(-2, 2, (m, 1)))).astype(np.float32)
    x = (y[rng.integers(0, m, n)] * (1 + 1e-4 * rng.standard_normal((n, D)))).astype(np.float32)
    y[:, 1::2] *= -1
    x[:, 1::2] *= -1                                        # (same products; operands of both signs in both MFMA k slots)
    s = mr.scores(x[:4], y)
    part = np.float32(0.5) * np.cumsum(y[0].astype(np.float64) ** 2)[-1] - np.cumsum(x[0].astype(np.float64) * y[0])
    assert (part[:-1] * part[1:] < 0).any() or np.abs(s).min() < 1e-3 * np.abs(y).max() ** 2      # partial sums change sign / cancel
    check_against_ref(x[None], y[None], 16, np.float32)
    a = knn_features(dev(x), dev(y), 16, _form="mfma")
    b = knn_features(dev(x), dev(y), 16, _form="valu")
    assert torch.equal(a[1], b[1]) and same(a[0], b[0])


# ------------------------------------------------------------------ 4
def gamma(nn, u):
    return nn * u / (1 - nn * u)


@pytest.mark.parametrize("kind", ["gaussian", "unit", "near_duplicates"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_against_the_truth(kind, dtype):
    rng = np.random.default_rng(14)
    n, m, D, k = 70, 400, 48, 8
    x, y = descr(rng, n, m, D, dtype)
    if kind == "unit":
        x, y = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(dtype), (y / np.linalg.norm(y, axis=1, keepdims=True)).astype(dtype)
    if kind == "near_duplicates":
        y = (y[:1] + 1e-6 * rng.standard_normal((m, D))).astype(dtype)
        x = (y[:1] + 1e-6 * rng.standard_normal((n, D))).astype(dtype)
    u = UNIT[dtype]
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    D2 = ((xd[:, None, :] - yd[None, :, :]) ** 2).sum(-1)
    E = gamma(2 * D + 1, u) * (0.5 * (yd ** 2).sum(1)[None, :] + np.abs(xd) @ np.abs(yd).T)
    for form in forms(dtype):
        d2, idx = (t.cpu().numpy() for t in knn_features(dev(x), dev(y), k, _form=form))
        assert (idx >= 0).all()
        for i in range(n):
            out = np.setdiff1d(np.arange(m), idx[i])
            lhs = (0.5 * D2[i, idx[i]] - E[i, idx[i]])[:, None]
            assert (lhs <= (0.5 * D2[i, out] + E[i, out])[None, :]).all(), (form, i)
        got = np.take_along_axis(D2, idx, 1)
        assert (np.abs(d2.astype(np.float64) - got) <= gamma(D + 2, u) * got).all(), form


# ------------------------------------------------------------------ 5
def grad_case(dtype, hub, seed=15):
    rng = np.random.default_rng(seed)
    N, n, m, D, k = 2, 300, 90, 20, 4
    x, y = (np.stack(t) for t in zip(*[descr(rng, n, m, D, dtype) for _ in range(N)]))
    if hub:                                                 # every query's neighbours among 4 rows of y: in-degree 300 > 4 chunks of 64
        y[:, 4:] += 100.0
    g = rng.standard_normal((N, n, k)).astype(dtype)
    g[rng.random(g.shape) < 0.1] = 0
    return x, y, g, [n, n - 17], [m, m - 9]


def run_grads(x, y, g, x_rows, y_rows, k, det):
    fx, fy = dev(x).requires_grad_(True), dev(y).requires_grad_(True)
    d2, idx = knn_features(fx, fy, k, x_rows=torch.tensor(x_rows).cuda(), y_rows=torch.tensor(y_rows).cuda(), deterministic=det)
    gd = torch.where(torch.isfinite(d2), dev(g), torch.zeros((), dtype=d2.dtype, device="cuda"))      # a zero cotangent on a +inf slot
    gx, gy = torch.autograd.grad(d2, [fx, fy], gd)
    return d2.detach(), idx, gd, gx, gy


@pytest.mark.parametrize("hub", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gradients(dtype, hub):
    x, y, g, x_rows, y_rows = grad_case(dtype, hub)
    k, u = g.shape[2], UNIT[dtype]
    d2, idx, gd, gx, gy = run_grads(x, y, g, x_rows, y_rows, k, False)
    assert (idx[1, x_rows[1]:] == -1).all() and torch.isinf(d2[1, x_rows[1]:]).all()
    # float64 autograd on the kernel's own idx
    X, Y = dev(x).double().requires_grad_(True), dev(y).double().requires_grad_(True)
    live = idx >= 0
    bi = torch.arange(x.shape[0], device="cuda")[:, None, None]
    diff = X[:, :, None, :] - Y[bi, idx.clamp(min=0)]
    out = torch.where(live, (diff ** 2).sum(-1), torch.zeros((), dtype=torch.float64, device="cuda"))
    rgx, rgy = torch.autograd.grad(out, [X, Y], gd.double(), retain_graph=True)
    terms = (2 * gd.double()[..., None] * diff).abs() * live[..., None]                                     # (N, n, k, D)
    mag_x = terms.sum(2)
    mag_y = torch.zeros_like(Y).index_put_((bi.expand_as(idx), idx.clamp(min=0)), terms, accumulate=True)
    deg = torch.zeros(Y.shape[:2], dtype=torch.float64, device="cuda").index_put_((bi.expand_as(idx), idx.clamp(min=0)), live.double(), accumulate=True)
    if hub:
        assert deg[0, :4].max() > 4 * 64 and (deg[0, 4:] == 0).all()
    det = run_grads(x, y, g, x_rows, y_rows, k, True)
    assert same(det[0], d2) and torch.equal(det[1], idx) and same(det[3], gx)                               # the forward and gx: the default call's
    for got_x, got_y in ((gx, gy), (det[3], det[4])):
        assert torch.isfinite(got_x).all() and torch.isfinite(got_y).all()
        assert ((got_x.double() - rgx).abs() <= (k + 2) * u * mag_x).all()
        assert ((got_y.double() - rgy).abs() <= (deg[..., None] + 2) * u * mag_y).all()
        assert (got_y[(deg == 0)[..., None].expand_as(got_y)] == 0).all()                                   # rows nobody names
        assert (got_y[1, y_rows[1]:] == 0).all() and (got_x[1, x_rows[1]:] == 0).all()
    # deterministic: the restatement's order, bit for bit, and the same bytes run after run
    idx_h, g_h = idx.cpu().numpy(), gd.cpu().numpy()
    for b in range(x.shape[0]):
        assert same(det[4][b], dev(mr.grad_y_det_ref(g_h[b], idx_h[b], x[b], y[b], y_rows[b])))
        assert same(gx[b], dev(mr.grad_x_ref(g_h[b], idx_h[b], x[b], y[b])))
    for _ in range(2):
        again = run_grads(x, y, g, x_rows, y_rows, k, True)
        assert same(again[4], det[4]) and same(again[3], det[3]) and same(again[0], det[0])


# ------------------------------------------------------------------ 6
RULES = [dict(mutual=False), dict(mutual=True), dict(mutual=False, ratio=0.8), dict(mutual=False, max_d2=30.0), dict(mutual=True, ratio=0.9, max_d2=40.0),
         dict(mutual=False, ratio=1.0)]


@pytest.mark.parametrize("rules", RULES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_match_features_rules(dtype, rules):
    rng = np.random.default_rng(16)
    N, n, m, D = 3, 60, 45, 6
    x, y = (np.stack(t) for t in zip(*[descr(rng, n, m, D, dtype) for _ in range(N)]))
    x_rows, y_rows = [n, n - 20, n], [m, m - 5, 1]          # cloud 2: a single candidate -- the ratio test passes it
    ref = [mr.match_features_ref(x[b], y[b], x_rows[b], y_rows[b], **rules) for b in range(N)]
    fx, fy = dev(x).requires_grad_(True), dev(y).requires_grad_(True)
    idx, d2 = match_features(fx, fy, x_rows=torch.tensor(x_rows).cuda(), y_rows=torch.tensor(y_rows).cuda(), **rules)
    assert torch.equal(idx, dev(np.stack([r[0] for r in ref]))) and same(d2.detach(), dev(np.stack([r[1] for r in ref])))
    if rules.get("ratio") is not None and not rules["mutual"]:
        assert (idx[2] == 0).all()                          # (with the mutual check only the one query that row 0 names back stays)
    assert (idx[1, x_rows[1]:] == -1).all()
    kept = idx >= 0
    assert kept.any() and (~kept).any() if len(rules) > 1 or rules["mutual"] else kept.any()
    gx, = torch.autograd.grad(torch.where(kept, d2, torch.zeros_like(d2)).sum(), [fx])
    assert (gx[~kept] == 0).all() and (gx[kept] != 0).any() and torch.isfinite(gx).all()                    # rejected rows: exactly zero


def test_max_d2_on_the_boundary():
    rng = np.random.default_rng(17)
    x, y = descr(rng, 50, 40, 5, np.float32)
    d2, _ = knn_features(dev(x), dev(y), 1)
    edge = float(d2[:, 0].median())
    idx, _ = match_features(dev(x), dev(y), mutual=False, max_d2=edge)
    assert torch.equal(idx >= 0, d2[:, 0] <= edge) and (d2[:, 0] == edge).any()                              # the boundary value itself is kept
    below = float(np.nextafter(np.float32(edge), np.float32(0)))
    assert torch.equal(match_features(dev(x), dev(y), mutual=False, max_d2=below)[0] >= 0, d2[:, 0] < edge)


# ------------------------------------------------------------------ 7
def align_case(dtype, seed=18):
    rng = np.random.default_rng(seed)
    N, n, m = 2, 200, 230
    R, t = mc.rotation(0.5, [1.0, 2.0, -1.0]), np.array([0.3, 0.0, 0.0])
    x = rng.uniform(-0.5, 0.5, (N, n, 3))
    idx = np.stack([rng.permutation(m)[:n] for _ in range(N)])
    y = rng.uniform(-0.5, 0.5, (N, m, 3))
    for b in range(N):
        y[b, idx[b]] = x[b] @ R.T + t + 0.01 * rng.standard_normal((n, 3))
    idx[rng.random((N, n)) < 0.2] = -1
    w = rng.uniform(0.1, 1.0, (N, n))
    return x.astype(dtype), y.astype(dtype), idx.astype(np.int64), w.astype(dtype), [n, n - 30]


def kabsch_torch(x, y, idx, w, rows):
    """float64 autograd reference: T (4, 4) of one cloud through torch.linalg.svd"""
    w = torch.where((idx >= 0) & (torch.arange(x.shape[0], device=x.device) < rows), w, torch.zeros_like(w))
    yy = y[idx.clamp(min=0)]
    wn = w / w.sum()
    mx, my = (wn[:, None] * x).sum(0), (wn[:, None] * yy).sum(0)
    H = ((yy - my) * wn[:, None]).T @ (x - mx)
    U, _, Vt = torch.linalg.svd(H)
    S = torch.diag(torch.stack([torch.ones_like(H[0, 0]), torch.ones_like(H[0, 0]), torch.det(U) * torch.det(Vt)]))
    C = U @ S @ Vt
    T = torch.eye(4, dtype=x.dtype, device=x.device)
    return torch.cat((torch.cat((C, (my - C @ mx)[:, None]), 1), T[3:]), 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_align_correspondences(dtype):
    x, y, idx, w, rows = align_case(dtype)
    pose_bar, grad_bar = (1e-10, 1e-10) if dtype == np.float64 else (1e-4, 1e-3)
    xt, yt, wt = (dev(a).requires_grad_(True) for a in (x, y, w))
    T = align_correspondences(xt, yt, dev(idx), weight=wt, x_rows=torch.tensor(rows).cuda())
    assert T.shape == (2, 4, 4)
    G = dev(np.random.default_rng(19).standard_normal((2, 4, 4)).astype(dtype))
    gx, gy, gw = torch.autograd.grad((T * G).sum(), [xt, yt, wt])
    X, Y, W = (dev(a).double().requires_grad_(True) for a in (x, y, w))
    ref = torch.stack([kabsch_torch(X[b], Y[b], dev(idx)[b], W[b], rows[b]) for b in range(2)])
    rgx, rgy, rgw = torch.autograd.grad((ref * G.double()).sum(), [X, Y, W])
    for b in range(2):
        live = (idx[b] >= 0) & (np.arange(idx.shape[1]) < rows[b])
        C, r = mc.kabsch(x[b][live].astype(np.float64), y[b][idx[b][live]].astype(np.float64), w[b][live].astype(np.float64))
        assert np.abs(T[b, :3, :3].detach().cpu().numpy() - C).max() <= pose_bar and np.abs(T[b, :3, 3].detach().cpu().numpy() - r).max() <= pose_bar
    assert (T.detach().double() - ref.detach()).abs().max() <= pose_bar
    for got, want in ((gx, rgx), (gy, rgy), (gw, rgw)):
        assert torch.isfinite(got).all() and (got.double() - want).abs().max() <= grad_bar
    # zero-weight rows: their points and their idx change nothing, bit for bit
    x2, idx2 = x.copy(), idx.copy()
    dead = idx < 0
    x2[dead] += 3.0
    x2[1, rows[1]:] -= 5.0
    idx2[1, rows[1]:] = 7
    w2 = w.copy()
    w2[dead] = 9.0
    T2 = align_correspondences(dev(x2), dev(y), dev(idx2), weight=dev(w2), x_rows=torch.tensor(rows).cuda())
    assert same(T2, T.detach())
    Ts = align_correspondences(dev(x[0]), dev(y[0]), dev(idx[0]).to(torch.int32), weight=dev(w[0]))
    assert Ts.shape == (4, 4) and same(Ts, T[0].detach())


# ------------------------------------------------------------------ 8
def check_pipeline(cases, rows_x=None, rows_y=None):
    fx, fy, x, y = (dev(np.stack([c[key] for c in cases])) for key in ("fx", "fy", "x", "y"))
    fx.requires_grad_(True)
    x.requires_grad_(True)
    rx = None if rows_x is None else torch.tensor(rows_x).cuda()
    ry = None if rows_y is None else torch.tensor(rows_y).cuda()
    idx, d2 = match_features(fx, fy, x_rows=rx, y_rows=ry, mutual=True, ratio=0.8)
    for b, c in enumerate(cases):
        gt = c["gt"].copy()
        if rows_x is not None:
            gt[rows_x[b]:] = -1
        if rows_y is not None:
            gt[gt >= rows_y[b]] = -1
        assert torch.equal(idx[b], dev(gt)), b              # exactly the ground truth on the kept rows, -1 on the replaced ones
    T0 = align_correspondences(x, y, idx, weight=torch.exp(-d2), x_rows=rx)
    # against the TRUE pose the fit is limited by the 0.005 noise of the points, not by the arithmetic: about 400 pairs in a unit cube give
    # a standard error of 0.005 / sqrt(400) = 2.5e-4 per component; 8 of them.  (The float32 bar against the float64 fit: test_end_to_end.)
    for b, c in enumerate(cases):
        assert np.abs(T0[b, :3, :3].detach().cpu().numpy() - c["R"]).max() <= 2e-3 and np.abs(T0[b, :3, 3].detach().cpu().numpy() - c["t"]).max() <= 2e-3
    g0, = torch.autograd.grad(T0.sum(), [fx], retain_graph=True)
    assert torch.isfinite(g0).all() and (g0 != 0).any()     # the descriptors are reached through d2 (the weights)
    out = ICP(icp_type="pt2pt", max_iterations=20, tolerance=1e-9).icp(x, y, T_init=T0, source_rows=rx, target_rows=ry)
    T = out["T"]
    # ICP matches EVERY source row to its nearest target: up to 10 % of the rows have lost their true partner (ragged target rows) and pull
    # towards a neighbour at most one point spacing (0.1) away: a bias of at most 0.1 * 0.1 = 1e-2 if they all pulled one way
    for b, c in enumerate(cases):
        assert np.abs(T[b, :3, :3].detach().cpu().numpy() - c["R"]).max() <= 1e-2 and np.abs(T[b, :3, 3].detach().cpu().numpy() - c["t"]).max() <= 1e-2
    T.sum().backward()
    assert torch.isfinite(x.grad).all() and (x.grad != 0).any()
    assert fx.grad is None or torch.isfinite(fx.grad).all()
    return T0


def test_end_to_end():
    c = mc.end_to_end(seed=0)
    T0 = check_pipeline([c])
    live = c["gt"] >= 0                                     # the float32 pose bar of test 7 against the Kabsch fit of the true pairs
    fx, fy = dev(c["fx"]), dev(c["fy"])
    idx, d2 = match_features(fx, fy, mutual=True, ratio=0.8)
    Tu = align_correspondences(dev(c["x"]), dev(c["y"]), idx)
    C, r = mc.kabsch(c["x"][live].astype(np.float64), c["y"][c["gt"][live]].astype(np.float64), np.ones(int(live.sum())))
    assert np.abs(Tu[:3, :3].cpu().numpy() - C).max() <= 1e-4 and np.abs(Tu[:3, 3].cpu().numpy() - r).max() <= 1e-4
    assert T0.shape == (1, 4, 4)


def test_end_to_end_batch_with_ragged_rows():
    check_pipeline([mc.end_to_end(seed=s) for s in (1, 2, 3)], rows_x=[500, 430, 500], rows_y=[600, 600, 540])


# ------------------------------------------------------------------ 9
@pytest.mark.parametrize("det", [False, True])
def test_captured_forward_and_backward(det):
    def data(seed):
        rng = np.random.default_rng(seed)
        x, y = descr(rng, 70, 130, 24, np.float32)
        return {"x": dev(x[None]), "y": dev(y[None]), "g": dev(rng.standard_normal((1, 70, 4)).astype(np.float32))}

    def run(s):
        fx, fy = s["x"].detach().requires_grad_(True), s["y"].detach().requires_grad_(True)
        d2, idx = knn_features(fx, fy, 4, deterministic=det)
        gx, gy = torch.autograd.grad(d2, [fx, fy], s["g"])
        return d2.detach(), idx, gx, gy
    static = data(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(static)
    for seed in (2, 3):
        fresh = data(seed)
        for key, t in fresh.items():
            static[key].copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(fresh)
        for i, (a, b) in enumerate(zip(captured, eager)):
            if i == 3 and not det:                          # atomics: the order, and so the last bits, differ from run to run
                assert torch.allclose(a, b, rtol=1e-5, atol=1e-5)
            else:
                assert same(a, b), (seed, i)
