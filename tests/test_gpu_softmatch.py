"""soft_match_features on the MI355X (dicp_amd/match.py; csrc/softmatch.hip).

1  the forward (out, prob) and the three gradients within the error model of tests/softmatch_ref.py against its float64 reference, idx
   index for index -- float64, and float32 in both forms (matrix cores and vector unit) -- around the 32-row tile, the 16-row block, every
   LDS stage edge of the matrix-core form as built, odd D, one channel pair and the cap, every C capacity, four temperatures; ragged
   batches with a cloud of 0 rows on each side and garbage in the pad rows; lists and CPU tensors;
2  designed inputs: a maximum that rises at every step, one first met in the last row of the last tile, equal maxima in two tiles and in
   a tile's two lane halves, |x|^2 / tau beyond exp's range, duplicate rows, non-finite rows on both sides, exact mass on one row;
3  idx against knn_features(k=1) on every case, the two float32 forms against each other;
4  the bytes of three runs on a hub and on a uniform layout;  5  soft matches -> align_correspondences -> backward against float64
   autograd of the dense composition;  6  forward + backward in a captured graph.

Figures (the largest |error| / bound per family): profiles/r28_softmatch_edges.txt.
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.match import align_correspondences, knn_features, soft_match_features

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_cases as mc  # noqa: E402
import softmatch_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

TD = {np.float32: torch.float32, np.float64: torch.float64}
OUTS = ("out", "prob", "gfx", "gfy", "gvalues")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and (torch.equal(bits(a), bits(b)) if a.dtype.is_floating_point else torch.equal(a, b))


def forms(dtype):
    return ("mfma", "valu") if dtype == np.float32 else (None,)


def run(fx, fy, values, tau, cot=None, form=None, x_rows=None, y_rows=None):
    """numpy (n, D) / (N, n, D) ... -> dict of torch tensors on the device: out, idx, prob[, gfx, gfy, gvalues]"""
    x, y, v = (dev(t).requires_grad_(cot is not None) for t in (fx, fy, values))
    kw = {}
    if x_rows is not None:
        kw = dict(x_rows=torch.tensor(x_rows), y_rows=torch.tensor(y_rows))
    out, idx, prob = soft_match_features(x, y, v, tau, return_best=True, _form=form, **kw)
    res = {"out": out.detach(), "idx": idx, "prob": prob}
    assert not idx.requires_grad and not prob.requires_grad
    if cot is not None:
        res["gfx"], res["gfy"], res["gvalues"] = torch.autograd.grad(out, [x, y, v], dev(cot))
    return res


def held(got, fx, fy, values, tau, cot, form, x_rows=None, y_rows=None, what=""):
    """one cloud of a result against the reference under the model -> the worst ratios; asserts"""
    g = {k: t.cpu().numpy() for k, t in got.items()}
    res = sr.hold(g, fx, fy, values, tau, x_rows, y_rows, cot, form="mfma" if form == "mfma" else "valu")
    worst = {k: v[1] for k, v in res.items()}
    print("%s form=%s worst |err| / bound: %s" % (what, form, {k: "%.3f" % w for k, w in worst.items()}))
    assert all(v[0] for v in res.values()), (what, form, worst)
    return worst


def check_case(fx, fy, values, tau, cot, what):
    """every form of the dtype on one cloud: the model, knn_features' index, the forms against each other"""
    dtype = fx.dtype.type
    got = {}
    for form in forms(dtype):
        got[form] = run(fx, fy, values, tau, cot, form)
        held(got[form], fx, fy, values, tau, cot, form, what=what)
        _, ki = knn_features(dev(fx), dev(fy), k=1)
        assert torch.equal(got[form]["idx"], ki[:, 0]), (what, form)
    if dtype == np.float32:
        a, b = got["mfma"], got["valu"]
        assert torch.equal(a["idx"], b["idx"])
        ref = sr.reference(fx, fy, values, tau, cot=cot)
        bm, bv = sr.bounds(fx, fy, values, tau, ref, cot, "mfma"), sr.bounds(fx, fy, values, tau, ref, cot, "valu")
        for k in OUTS:
            assert np.all(np.abs(a[k].cpu().numpy().astype(np.float64) - b[k].cpu().numpy()) <= bm[k] + bv[k]), (what, k)
        auto = run(fx, fy, values, tau, cot, None)
        for k in OUTS + ("idx",):
            assert same(auto[k], a[k]), (what, k)                   # float32 without _form is the matrix-core form
    return got


# n, m, D, C, tau: the stage of the matrix-core form holds 256 rows up to D = 32, 224 at D = 33 / 34, 128 at 64, 64 at 128, 32 from 129 on
CASES32 = [
    (1, 1, 1, 1, 1.0), (31, 31, 2, 3, 0.1), (32, 32, 3, 6, 0.01), (33, 33, 31, 8, 10.0), (127, 255, 32, 3, 0.1), (128, 256, 32, 3, 0.01),
    (129, 257, 32, 1, 1.0), (33, 513, 33, 3, 0.1), (32, 223, 33, 6, 1.0), (31, 224, 33, 3, 10.0), (33, 225, 33, 8, 0.01), (33, 127, 64, 3, 0.1),
    (32, 128, 64, 1, 0.01), (31, 129, 64, 6, 1.0), (33, 63, 128, 3, 0.1), (32, 64, 128, 3, 1.0), (31, 65, 128, 8, 0.1), (33, 31, 255, 3, 1.0),
    (129, 33, 255, 3, 0.1), (32, 32, 256, 6, 0.1), (127, 33, 256, 3, 0.01), (1, 513, 3, 3, 0.1),
]
# float64 runs the vector kernels at every size; its reference is exact rational arithmetic per element, so the shapes stay small
CASES64 = [
    (1, 1, 1, 1, 1.0), (31, 33, 3, 3, 0.1), (33, 31, 31, 6, 0.01), (32, 257, 2, 3, 1.0), (33, 65, 33, 8, 10.0), (31, 33, 64, 3, 0.1),
    (5, 33, 256, 3, 1.0), (129, 32, 3, 1, 0.01), (3, 17, 255, 6, 0.1), (2, 513, 1, 3, 0.1), (127, 16, 2, 3, 1.0), (128, 15, 3, 8, 10.0),
]


@pytest.mark.parametrize("case", CASES32)
def test_float32_within_the_bound(case):
    n, m, D, C, tau = case
    fx, fy, values, cot = sr.random_case(n, m, D, C, np.float32, seed=n * 7 + m * 3 + D)
    check_case(fx, fy, values, tau, cot, "f32 %s" % (case,))


@pytest.mark.parametrize("case", CASES64)
def test_float64_within_the_bound(case):
    n, m, D, C, tau = case
    fx, fy, values, cot = sr.random_case(n, m, D, C, np.float64, seed=n * 7 + m * 3 + D)
    check_case(fx, fy, values, tau, cot, "f64 %s" % (case,))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ragged_lists_and_cpu_tensors(dtype):
    N, n, m, D, C, tau = 3, 40, 70, 16 if dtype == np.float32 else 4, 3, 0.1
    xr, yr = [40, 0, 25], [70, 33, 0]                               # a cloud of 0 rows on each side in turn
    parts = [sr.random_case(n, m, D, C, dtype, seed=50 + b) for b in range(N)]
    fx, fy, values, cot = (np.stack([p[i] for p in parts]) for i in range(4))
    for b in range(N):                                              # garbage in the pad rows
        fx[b, xr[b]:] = np.nan if b % 2 else 1e30
        fy[b, yr[b]:] = 1e30 if b % 2 else np.nan
        values[b, yr[b]:] = np.nan
        cot[b, xr[b]:] = np.nan
    for form in forms(dtype):
        got = run(fx, fy, values, tau, cot, form, xr, yr)
        for b in range(N):
            held({k: t[b] for k, t in got.items()}, fx[b], fy[b], values[b], tau, cot[b], form, xr[b], yr[b], what="ragged cloud %d" % b)
            assert torch.all(got["out"][b, xr[b]:] == 0) and torch.all(got["idx"][b, xr[b]:] == -1) and torch.all(got["prob"][b, xr[b]:] == 0)
            assert torch.all(got["gfx"][b, xr[b]:] == 0) and torch.all(got["gfy"][b, yr[b]:] == 0) and torch.all(got["gvalues"][b, yr[b]:] == 0)
        _, ki = knn_features(dev(fx), dev(fy), k=1, x_rows=torch.tensor(xr), y_rows=torch.tensor(yr))
        assert torch.equal(got["idx"], ki[..., 0])
        if form != "valu":
            # lists of CPU tensors: the same bytes per cloud, on the CPU, gradients included
            lx, ly, lv = ([torch.from_numpy(t[b, :r[b]].copy()).requires_grad_(True) for b in range(N)] for t, r in ((fx, xr), (fy, yr), (values, yr)))
            out, idx, prob = soft_match_features(lx, ly, lv, tau, return_best=True)
            assert all(not t.is_cuda for t in out + idx + prob)
            sum((o * torch.from_numpy(cot[b, :xr[b]])).sum() for b, o in enumerate(out)).backward()
            for b in range(N):
                assert same(out[b].detach(), got["out"][b, :xr[b]].cpu()) and torch.equal(idx[b], got["idx"][b, :xr[b]].cpu())
                assert same(prob[b], got["prob"][b, :xr[b]].cpu())
                assert same(lx[b].grad, got["gfx"][b, :xr[b]].cpu()) and same(ly[b].grad, got["gfy"][b, :yr[b]].cpu())
                assert same(lv[b].grad, got["gvalues"][b, :yr[b]].cpu())
            # a single CPU table
            o1 = soft_match_features(torch.from_numpy(fx[0]), torch.from_numpy(fy[0]), torch.from_numpy(values[0]), tau)
            assert not o1.is_cuda and same(o1, got["out"][0].cpu())


# ------------------------------------------------------------------ designed inputs
def line_case(m, dtype, order):
    """rows of fy on a line, the queries beside its start: the scores strictly monotone in j"""
    fx, fy, values, cot = sr.random_case(37, m, 2, 3, dtype, 4)
    far, near = (3.0, 1.0) if order == "descending" else (1.0, 3.0)
    fy[:, 0], fy[:, 1] = np.linspace(far, near, m), 0.0
    fx[:, 0], fx[:, 1] = 0.9, 0.01 * fx[:, 1]
    return fx, fy, values, cot


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_designed_maxima(dtype):
    m = 257 if dtype == np.float32 else 70
    # the distance falls with j: the maximum rises at every step, and is first met in the last row of the last tile
    fx, fy, values, cot = line_case(m, dtype, "descending")
    got = check_case(fx, fy, values, 0.05, cot, "descending")
    assert all(torch.all(g["idx"] == m - 1) for g in got.values())
    # equal maxima in two tiles (rows 5 and 40) and in the two lane halves of one tile (rows 1 and 5); duplicates: idx is the lowest
    fx, fy, values, cot = sr.random_case(37, m, 8, 6, dtype, 5)
    fx[:] = fy[5] + 0.05 * fx
    fy[40] = fy[5]
    got = check_case(fx, fy, values, 0.1, cot, "equal maxima in two tiles")
    assert all(torch.all(g["idx"] == 5) for g in got.values())
    fy[1] = fy[5]
    got = check_case(fx, fy, values, 0.1, cot, "equal maxima in two lane halves")
    assert all(torch.all(g["idx"] == 1) for g in got.values())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_large_norm_at_small_temperature(dtype):
    """|x|^2 = 32 at tau = 0.01: the logits are near +3200, beyond exp's range without the running maximum"""
    n, m, D = 33, 70 if dtype == np.float32 else 20, 32
    fx, fy, values, cot = sr.random_case(n, m, D, 3, dtype, 6)
    fy[:] = 1.0 + 0.05 * fy
    fx[:] = 1.0
    got = check_case(fx, fy, values, 0.01, cot, "|x|^2 = 32")
    for g in got.values():
        assert all(bool(torch.isfinite(g[k]).all()) for k in OUTS)
        assert float(g["out"].abs().max()) > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_non_finite_rows(dtype):
    """a NaN channel in the last row of fy and an inf channel in the last row of fx: that row is nobody's candidate, that query is zeroed,
    and nobody else changes bit for bit against the call without them"""
    n, m, D, C, tau = 34, 66 if dtype == np.float32 else 20, 5, 3, 0.1
    fx, fy, values, cot = sr.random_case(n, m, D, C, dtype, 7)
    fy[m - 1, 2] = np.nan
    fx[n - 1, 0] = np.inf
    for form in forms(dtype):
        a = run(fx, fy, values, tau, cot, form)
        held(a, fx, fy, values, tau, cot, form, what="non-finite rows")
        b = run(fx[:n - 1], fy[:m - 1], values[:m - 1], tau, cot[:n - 1], form)
        assert a["idx"][n - 1] == -1 and torch.all(a["out"][n - 1] == 0) and a["prob"][n - 1] == 0 and torch.all(a["gfx"][n - 1] == 0)
        assert torch.all(a["gfy"][m - 1] == 0) and torch.all(a["gvalues"][m - 1] == 0) and not torch.any(a["idx"] == m - 1)
        for k in ("out", "idx", "prob", "gfx"):
            assert same(a[k][:n - 1], b[k]), (form, k)
        for k in ("gfy", "gvalues"):
            assert same(a[k][:m - 1], b[k]), (form, k)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_mass_on_one_row(dtype):
    """fx_i == fy_j bit for bit, every other row at d2 >= 1, tau = 1e-3: every other exponent is below -750 and underflows in both dtypes"""
    rng = np.random.default_rng(8)
    m, D, C = 81, 4, 6
    fy = np.stack(np.meshgrid(*([np.arange(3.0)] * D), indexing="ij"), axis=-1).reshape(-1, D).astype(dtype)      # distinct lattice points
    rng.shuffle(fy)
    pick = rng.integers(0, m, 50)
    fx = fy[pick].copy()
    values = rng.uniform(-1, 1, (m, C)).astype(dtype)
    for form in forms(dtype):
        got = run(fx, fy, values, 1e-3, None, form)
        assert torch.equal(got["idx"].cpu(), torch.from_numpy(pick))
        assert same(got["out"].cpu(), torch.from_numpy(values[pick])) and torch.all(got["prob"] == 1)


# ------------------------------------------------------------------ the same bytes on every run
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["hub", "uniform"])
def test_bit_reproducible(dtype, layout):
    N, n, m, D, C = 2, 300, 200, 24, 3
    rng = np.random.default_rng(9)
    fy = rng.standard_normal((N, m, D))
    if layout == "hub":                                            # every query's mass is on 16 rows of fy
        fx = fy[:, rng.integers(0, 16, n)] + 0.05 * rng.standard_normal((N, n, D))
    else:
        fx = rng.standard_normal((N, n, D))
    fx, fy, values, cot = (t.astype(dtype) for t in (fx, fy, rng.uniform(-1, 1, (N, m, C)), rng.standard_normal((N, n, C))))
    runs = [run(fx, fy, values, 0.5, cot) for _ in range(3)]
    for r in runs[1:]:
        for k in OUTS + ("idx",):
            assert same(r[k], runs[0][k]), k
    assert all(float(runs[0][k].abs().max()) > 0 for k in OUTS)


# ------------------------------------------------------------------ soft matches -> the closed-form fit -> backward
def kabsch_torch(x, y, w, transposed):
    """the weighted Procrustes fit in float64 torch -> (C, r); transposed: the SVD of the covariance's transpose (another route to the same C)"""
    ws = w.sum()
    mx, my = (w[:, None] * x).sum(0) / ws, (w[:, None] * y).sum(0) / ws
    H = ((x - mx) * w[:, None]).T @ (y - my)
    if transposed:
        V, _, Ut = torch.linalg.svd(H.T)
        U = Ut.T
    else:
        U, _, Vt = torch.linalg.svd(H)
        V = Vt.T
    d = torch.sign(torch.det(V @ U.T))
    Cm = V @ torch.diag(torch.stack((torch.ones_like(d), torch.ones_like(d), d))) @ U.T
    return Cm, my - Cm @ mx


def dense_composition(a, tau, second):
    """float64 autograd of softmax(-d2 / tau) @ y -> fit (weight: the row maximum, no gradient) -> sum of T, on the CPU.  second: the
    same function by another route (the score form under a log-sum-exp, the transposed SVD)"""
    fx, fy, y = (torch.tensor(a[k].astype(np.float64), requires_grad=True) for k in ("fx", "fy", "y"))
    x = torch.tensor(a["x"].astype(np.float64))
    if second:
        l = (-2.0 / tau) * (0.5 * (fy * fy).sum(-1)[None, :] - fx @ fy.T)
        p = torch.exp(l - torch.logsumexp(l, dim=1, keepdim=True))
    else:
        d = fx[:, None, :] - fy[None, :, :]
        p = torch.softmax(-(d * d).sum(-1) / tau, dim=1)
    soft = p @ y
    Cm, r = kabsch_torch(x, soft, p.max(dim=1).values.detach(), second)
    (Cm.sum() + r.sum() + 1.0).backward()
    return [t.grad.numpy() for t in (fx, fy, y)], Cm.detach().numpy(), r.detach().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_composition_reaches_the_descriptors(dtype):
    tau = 8.0
    a = mc.end_to_end(seed=0, n=500, m=600, D=32, dtype=dtype)
    fx, fy, y = (dev(a[k]).requires_grad_(True) for k in ("fx", "fy", "y"))
    x = dev(a["x"])
    soft, idx, prob = soft_match_features(fx, fy, y, tau, return_best=True)
    T = align_correspondences(x, soft, torch.arange(500, device="cuda"), weight=prob)
    T.sum().backward()
    grads = [t.grad.cpu().numpy() for t in (fx, fy, y)]
    for g in grads:
        assert np.isfinite(g).all() and np.abs(g).max() > 0
    if dtype == np.float32:
        return                                                      # (the operator-level bound above is the float32 check)
    ref, Cm, r = dense_composition(a, tau, False)
    ref2, _, _ = dense_composition(a, tau, True)
    assert np.allclose(T[:3, :3].detach().cpu().numpy(), Cm, atol=1e-9) and np.allclose(T[:3, 3].detach().cpu().numpy(), r, atol=1e-9)
    for name, g, r1, r2 in zip(("fx", "fy", "values"), grads, ref, ref2):
        scale = np.abs(r1).max()
        own = np.abs(r1 - r2).max() / scale                         # two float64 evaluations of the reference against each other
        err = np.abs(g - r1).max() / scale
        print("composition %s.grad: max|grad| %.3e, reference against itself %.3e, kernel against reference %.3e, ratio %.2f"
              % (name, scale, own, err, err / max(own, 1e-300)))
        assert err <= 16 * own, (name, err, own)


# ------------------------------------------------------------------ a captured graph
def test_captured_forward_and_backward():
    def data(seed):
        fx, fy, values, cot = sr.random_case(70, 130, 24, 3, np.float32, seed)
        return {"x": dev(fx[None]), "y": dev(fy[None]), "v": dev(values[None]), "g": dev(cot[None])}

    def once(s):
        fx, fy, v = (s[k].detach().requires_grad_(True) for k in ("x", "y", "v"))
        out, idx, prob = soft_match_features(fx, fy, v, 0.1, return_best=True)
        gx, gy, gv = torch.autograd.grad(out, [fx, fy, v], s["g"])
        return out.detach(), idx, prob, gx, gy, gv
    static = data(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            once(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = once(static)
    for seed in (2, 3):
        fresh = data(seed)
        for key, t in fresh.items():
            static[key].copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = once(fresh)
        for i, (a, b) in enumerate(zip(captured, eager)):
            assert same(a, b), (seed, i)
