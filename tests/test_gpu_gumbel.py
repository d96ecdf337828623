"""The fused Gumbel-softmax correspondence (csrc/kernels_soft_svd.h: gumbel_fwd_kernel, gumbel_bwd_q_kernel, gumbel_bwd_t_kernel) and the soft
loop around it, held value by value to tests/gumbel_ref.py: a float64 reference, a first-order error model with safety factor 1 and a numpy
restatement of the in-kernel noise.  Every tolerance here is the model's bound, an exact equality, or the 1e-12 * max rule of the one atomic sum.
`-m gpu`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gumbel_ref as G  # noqa: E402

from dicp_amd import _ops  # noqa: E402
from dicp_amd.ICP import ICP  # noqa: E402
from dicp_amd.synthetic import make_pairs  # noqa: E402
from oracle import dicp_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float64]
_SETS = {}


def npy(t):
    return t.detach().cpu().numpy()


def dev(a, dtype, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).requires_grad_(grad)


def run_op(x, y, U, cot, eps, tau, dtype, seed=None):
    xd, yd = dev(x, dtype, True), dev(y, dtype, True)
    out = _ops.gumbel_nn(xd, yd, eps, tau, U=None if U is None else dev(U, dtype), seed=seed)
    out.backward(dev(cot, dtype))
    return {"out": npy(out), "gx": npy(xd.grad), "gy": npy(yd.grad)}, (out.detach(), xd.grad, yd.grad)


def held(x, y, U, cot, eps, tau, dtype, what):
    got, _ = run_op(x, y, U, cot, eps, tau, dtype)
    res = G.hold(got, x, y, U, eps, tau, dtype, cot)
    print(what, {k: (v[0], "%.4f" % v[1], v[2]) for k, v in res.items()})
    bad = {k: v for k, v in res.items() if not v[0]}
    assert not bad, (what, bad)


def designed(dtype, **kw):
    key = (str(dtype),) + tuple(sorted(kw.items()))
    if key not in _SETS:
        _SETS[key] = G.designed_sets(dtype, **kw)
    return _SETS[key]


# ------------------------------------------------------------------ 1. the operator against the model, injected noise
# BLOCK = 256 and GUM_TILE = 512: the (3, 300, 1100) case at both c, and the edge values of n and m one at a time.  At the full shape c = 3 crosses every tau
# with both eps and takes the clouds 100 and 2500 units from the origin at the largest and the smallest tau; the edge shapes take one mild and one sharp setting.
FULL = [(3, tau, eps, 0.0) for tau in (0.5, 0.1, 0.05, 0.01) for eps in (1e-10, 1e-20)] + [(3, tau, 1e-20, off) for tau in (0.5, 0.01) for off in (100.0, 2500.0)] \
    + [(6, tau, 1e-20, off) for tau in (0.5, 0.05) for off in (0.0, 2500.0)]
EDGES = [(n, 1100) for n in (1, 255, 256, 257)] + [(300, m) for m in (1, 2, 511, 512, 513, 1025)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,tau,eps,off", FULL)
def test_operator_within_the_model_full_shape(dtype, c, tau, eps, off):
    x, y, U, cot = G.random_set(3, 300, 1100, c, dtype, 1, off)
    held(x, y, U, cot, eps, tau, dtype, ("full", c, tau, eps, off))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", EDGES)
def test_operator_within_the_model_edge_shapes(dtype, n, m):
    for k, (c, tau, eps, off) in enumerate(((3, 0.1, 1e-20, 0.0), (6, 0.01, 1e-10, 100.0))):
        x, y, U, cot = G.random_set(3, n, m, c, dtype, 20 + k, off)
        held(x, y, U, cot, eps, tau, dtype, ("edge", n, m, c, tau, eps, off))


# ------------------------------------------------------------------ 2. designed inputs
NAMES = ["near_j%d" % j for j in (0, 511, 512, 513, 1023, 1024, 1099)] + ["ascending", "descending", "max_at_512", "equal_maxima", "noise_edges_eps1e-10", "noise_edges_eps1e-20"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_designed_inputs_within_the_model(dtype, name):
    """tests/gumbel_ref.py: designed_sets.  A structural fault on these leaves the bound (tests/test_gumbel_ref.py shows it for five of them)."""
    x, y, U, cot, eps, tau = designed(dtype)[name]
    held(x, y, U, cot, eps, tau, dtype, name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_designed_inputs_with_normals(dtype):
    """c = 6, columns 3:6 unit normals beside coordinates of another scale, one tile and one row past it (n = 257, m = 513)"""
    sets = designed(dtype, n=257, m=513, c=6)
    for name in ("near_j512", "equal_maxima", "noise_edges_eps1e-10", "ascending"):
        x, y, U, cot, eps, tau = sets[name]
        held(x, y, U, cot, eps, tau, dtype, name + "/c6")


# ------------------------------------------------------------------ 3. in-kernel noise is the injected restatement
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [3, 6])
@pytest.mark.parametrize("seed", [0, 1, 2 ** 31 - 2, 0xFFFFFFFF])
def test_in_kernel_noise_is_the_restated_hash(dtype, c, seed):
    """The three kernels differ between U = None and an injected U only in where u comes from, and none uses atomics: injecting hash_uniform(seed)
    gives the same bits.  Pins the forward key, both backward keys, the cloud term, i >= 256 and j >= 512."""
    N, n, m = 3, 300, 1100
    x, y, _, cot = G.random_set(N, n, m, c, dtype, 3)
    _, a = run_op(x, y, None, cot, 1e-20, 0.1, dtype, seed=seed)
    _, b = run_op(x, y, G.hash_uniform(seed, N, n, m), cot, 1e-20, 0.1, dtype)
    for p, q, what in zip(a, b, ("out", "gx", "gy")):
        assert torch.equal(p, q), (what, float((p - q).abs().max()))


# ------------------------------------------------------------------ 4. the soft loop regenerates what it drew
def _soft_icp(icp_type, K, const_iter, tolerance=1e-14):
    icp = ICP(icp_type=icp_type, differentiable=True, max_iterations=K, tolerance=tolerance)
    icp.const_iter = const_iter
    icp.nn.use_gumbel, icp.nn.eps, icp.nn.tau = True, 1e-10, 0.1
    return icp


def _loop_run(icp, src, tgt, T0, gT, **kw):
    s, t = src.clone().requires_grad_(True), tgt.clone().requires_grad_(True)
    out = icp.icp(s, t, T0, **kw)
    ((out["T"] * gT).sum() + out["deltas"].sum() + 0.01 * out["weights"].sum()).backward()
    return out, s.grad, t.grad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("icp_type", ["pt2pl", "pt2pt"])
@pytest.mark.parametrize("const_iter", [True, False])
def test_soft_loop_regenerates_its_noise(dtype, icp_type, const_iter):
    """In-kernel noise after torch.manual_seed against the same call with hash_uniform(seed_k) injected, the seeds read from knn_stats["gumbel_seeds"]:
    the backward must read seeds[k], nbr_k and lse_k as the forward wrote them.  No sum of this path has more than one writer per address (the neighbour rows
    are one per source point), so everything is compared bit for bit but the target gradient in float64, which keeps the existing rule of its atomic sums
    (1e-12 of the largest entry).  Tolerance mode: frozen clouds and trimmed histories."""
    N, n, m, K = 3, 300, 600, 3
    src, tgt = make_pairs(N, n, m, seed=61, dtype=dtype, max_rot=0.03, max_trans=0.1)
    src, tgt = src.to(DEV), (tgt if icp_type == "pt2pl" else tgt[:, :, :3].contiguous()).to(DEV)
    T0 = torch.eye(4, dtype=dtype, device=DEV).repeat(N, 1, 1)
    gT = torch.randn((N, 4, 4), generator=torch.Generator().manual_seed(2), dtype=torch.float64).to(dtype).to(DEV)
    kw = dict(trim_dist=5.0, loss_fn={"name": "huber", "metric": 1.0}, dim=3)
    tol = 1e-14 if const_iter else 5e-2
    icp = _soft_icp(icp_type, K, const_iter, tol)
    torch.manual_seed(77)
    a, ga_s, ga_t = _loop_run(icp, src, tgt, T0, gT, **kw)
    seeds = icp.knn_stats["gumbel_seeds"]
    torch.manual_seed(77)
    assert seeds == tuple(int(v) & 0xFFFFFFFF for v in torch.randint(0, 2 ** 31 - 1, (K,)).tolist())
    icp2 = _soft_icp(icp_type, K, const_iter, tol)
    icp2.nn._inject_U = [torch.tensor(G.hash_uniform(s, N, n, m), dtype=dtype, device=DEV) for s in seeds]
    b, gb_s, gb_t = _loop_run(icp2, src, tgt, T0, gT, **kw)
    for key in ("T", "deltas", "weights", "costs", "pc"):
        assert a[key].shape == b[key].shape and torch.equal(a[key], b[key]), key
    assert torch.equal(a["stats"]["iterations"], b["stats"]["iterations"])
    assert torch.equal(ga_s, gb_s)
    assert bool(torch.isfinite(ga_t).all()) and float(ga_t.abs().max()) > 0
    if dtype == torch.float64:
        assert float((ga_t - gb_t).abs().max()) <= 1e-12 * float(gb_t.abs().max())
    else:
        assert torch.equal(ga_t, gb_t)


# ------------------------------------------------------------------ 5. the loop's neighbours against the model
@pytest.mark.parametrize("icp_type", ["pt2pl", "pt2pt"])
def test_soft_loop_neighbours_within_the_model(icp_type):
    """One iteration of the soft loop in float32 at (3, 300, 600): the neighbour rows the loop saved for its backward are held to gumbel_ref on the loop's own
    transformed source (transform_points of the start pose: the same kernel).  The accumulate that follows is held by tests/test_gpu_point_math.py."""
    N, n, m, dtype = 3, 300, 600, torch.float32
    src, tgt = make_pairs(N, n, m, seed=62, dtype=dtype, max_rot=0.03, max_trans=0.1)
    src, tgt = src.to(DEV).requires_grad_(True), (tgt if icp_type == "pt2pl" else tgt[:, :, :3].contiguous()).to(DEV)
    ang = 0.02
    T0 = torch.eye(4, dtype=dtype).repeat(N, 1, 1)
    T0[:, 0, 0] = T0[:, 1, 1] = float(np.cos(ang))
    T0[:, 0, 1], T0[:, 1, 0] = -float(np.sin(ang)), float(np.sin(ang))
    T0[:, :3, 3] = torch.tensor([0.05, -0.02, 0.01])
    T0 = T0.to(DEV)
    U = G.hash_uniform(9, N, n, m)
    icp = _soft_icp(icp_type, 1, True)
    icp.nn._inject_U = [torch.tensor(U, dtype=dtype, device=DEV)]
    out = icp.icp(src, tgt, T0, trim_dist=5.0, loss_fn={"name": "huber", "metric": 1.0}, dim=3)
    saved = out["T"].grad_fn.saved_tensors
    nbr = [t for t in saved if t.dim() == 4 and tuple(t.shape) == (1, N, n, tgt.shape[2])]
    assert len(nbr) == 1
    x = npy(_ops.transform_points(src.detach(), T0)).astype(np.float64)
    y = npy(tgt).astype(np.float64)
    ref = G.reference(x, y, U, 1e-10, 0.1, dtype)
    ok, worst, at = G.compare(npy(nbr[0][0]), ref["out"], G.bounds(x, y, U, 1e-10, 0.1, dtype, ref=ref)["out"])
    print("loop neighbours", icp_type, worst, at)
    assert ok, (worst, at)


# ------------------------------------------------------------------ 6. ragged soft calls
SRC_ROWS, TGT_ROWS = (300, 257, 1), (600, 513, 2)


def _padded(kind, src, tgt):
    sp, tp = src.clone(), tgt.clone()
    for b in range(src.shape[0]):
        nb, mb = SRC_ROWS[b], TGT_ROWS[b]
        if kind == "copies":       # the target row nearest to query 0, and query 0 itself
            j = int(((tgt[b, :mb, :3] - src[b, 0]) ** 2).sum(-1).argmin())
            sp[b, nb:], tp[b, mb:] = src[b, 0], tgt[b, j]
        else:
            v = {"nan": float("nan"), "inf": float("inf"), "1e30": 1e30}[kind]
            sp[b, nb:], tp[b, mb:] = v, v
    return sp, tp


@pytest.mark.parametrize("icp_type,dtype", [("pt2pl", torch.float64), ("pt2pt", torch.float32)])
@pytest.mark.parametrize("kind", ["nan", "inf", "1e30", "copies"])
def test_ragged_soft_call_is_the_dense_calls(icp_type, dtype, kind):
    """A padded batch with source_rows / target_rows through the soft loop, whatever the pads hold: the forward equals, bit for bit, the three dense single-cloud
    calls on the truncated clouds with U[b, :n_b, :m_b] (the tiles start at j = 0: the operation order is the same); the gradients of the live rows equal theirs
    (the target's in float64 to 1e-12 of its largest entry), the gradients of every pad row are exactly 0, and nothing is non-finite (pc: on the clouds' own rows --
    a pad row of pc is the pose applied to whatever the pad holds; with non-finite pads the loss leaves pc out, because the adjoint of that last transform, which
    is not the soft loop's, multiplies a zero cotangent with the pad's coordinates)."""
    N, n, m, K = 3, 300, 600, 2
    src, tgt = make_pairs(N, n, m, seed=63, dtype=dtype, max_rot=0.03, max_trans=0.1)
    tgt = tgt if icp_type == "pt2pl" else tgt[:, :, :3].contiguous()
    sp, tp = _padded(kind, src, tgt)
    sp, tp = sp.to(DEV).requires_grad_(True), tp.to(DEV).requires_grad_(True)
    Us = [torch.tensor(G.hash_uniform(40 + k, N, n, m), dtype=dtype, device=DEV) for k in range(K)]
    T0 = torch.eye(4, dtype=dtype, device=DEV).repeat(N, 1, 1)
    gT = torch.randn((N, 4, 4), generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(dtype).to(DEV)
    kw = dict(trim_dist=5.0, loss_fn={"name": "huber", "metric": 1.0}, dim=3)
    with_pc = kind in ("1e30", "copies")

    def loss(out, g, rows):
        v = (out["T"] * g).sum() + out["deltas"].sum() + 0.01 * sum(out["weights"][b, :, :r].sum() for b, r in enumerate(rows))
        return v + 0.1 * sum((out["pc"][b, :r] ** 2).sum() for b, r in enumerate(rows)) if with_pc else v

    icp = _soft_icp(icp_type, K, True)
    icp.nn._inject_U = Us
    out = icp.icp(sp, tp, T0, source_rows=list(SRC_ROWS), target_rows=list(TGT_ROWS), **kw)
    loss(out, gT, SRC_ROWS).backward()
    for key in ("T", "deltas", "costs", "weights"):
        assert bool(torch.isfinite(out[key]).all()), key
    assert bool(torch.isfinite(sp.grad).all()) and bool(torch.isfinite(tp.grad).all())
    for b in range(N):
        nb, mb = SRC_ROWS[b], TGT_ROWS[b]
        s1 = src[b:b + 1, :nb].contiguous().to(DEV).requires_grad_(True)
        t1 = tgt[b:b + 1, :mb].contiguous().to(DEV).requires_grad_(True)
        one_icp = _soft_icp(icp_type, K, True)
        one_icp.nn._inject_U = [u[b:b + 1, :nb, :mb].contiguous() for u in Us]
        one = one_icp.icp(s1, t1, T0[b:b + 1], **kw)
        loss(one, gT[b:b + 1], (nb,)).backward()
        for key in ("T", "deltas", "costs"):
            assert torch.equal(out[key][b], one[key][0]), (key, b, float((out[key][b] - one[key][0]).abs().max()))
        r = 3 if icp_type == "pt2pt" else 1
        assert torch.equal(out["weights"][b, :, :nb * r], one["weights"][0]), ("weights", b)
        assert float(out["weights"][b, :, nb * r:].abs().sum()) == 0.0
        assert torch.equal(out["pc"][b, :nb], one["pc"][0]) and bool(torch.isfinite(out["pc"][b, :nb]).all()), ("pc", b)
        assert torch.equal(sp.grad[b, :nb], s1.grad[0]), ("source gradient", b, float((sp.grad[b, :nb] - s1.grad[0]).abs().max()))
        if dtype == torch.float64:
            assert float((tp.grad[b, :mb] - t1.grad[0]).abs().max()) <= 1e-12 * float(t1.grad.abs().max()), ("target gradient", b)
        else:
            assert torch.equal(tp.grad[b, :mb], t1.grad[0]), ("target gradient", b, float((tp.grad[b, :mb] - t1.grad[0]).abs().max()))
        assert bool((sp.grad[b, nb:] == 0).all()) and bool((tp.grad[b, mb:] == 0).all()), ("pad gradients", b)


def test_lists_keep_the_reference_padding(monkeypatch):
    """The same ragged clouds as LISTS: the reference pads the targets with copies of one far point and softmaxes over all of them, and so does the soft loop
    (it takes no row counts from a list).  Held to the oracle on the reference's own padded batch in float64, to the bar of smoke(): 1e-9 on the pose,
    1e-8 on the gradients."""
    N, n, m, K, dtype = 3, 300, 600, 2, torch.float64
    src, tgt = make_pairs(N, n, m, seed=63, dtype=dtype, max_rot=0.03, max_trans=0.1)
    S = [src[b, :SRC_ROWS[b]].contiguous() for b in range(N)]
    Tg = [tgt[b, :TGT_ROWS[b]].contiguous() for b in range(N)]
    Us = [torch.tensor(G.hash_uniform(50 + k, N, n, m)) for k in range(K)]
    kw = dict(trim_dist=5.0, loss_fn={"name": "huber", "metric": 1.0}, dim=3)
    icp = _soft_icp("pt2pl", K, True)
    sb, tb, Tb, wb = ICP(icp_type="pt2pl", differentiable=True, max_iterations=K, tolerance=1e-14).batch_size_handling(S, Tg, [torch.eye(4, dtype=dtype)] * N)
    draws = iter(Us)
    monkeypatch.setattr(torch, "rand", lambda *a, **k: next(draws))
    sc, tc = sb.clone().requires_grad_(True), tb.clone().requires_grad_(True)
    ref = O.icp_batched(sc, tc, Tb, wb, icp_type="pt2pl", differentiable=True, max_iterations=K, tolerance=1e-14, const_iter=True,
                        use_gumbel=True, gumbel_eps=1e-10, gumbel_tau=0.1, **kw)
    monkeypatch.undo()
    ref["T"].sum().backward()
    icp.nn._inject_U = [u.to(DEV) for u in Us]
    Sd, Td = [s.to(DEV).requires_grad_(True) for s in S], [t.to(DEV).requires_grad_(True) for t in Tg]
    out = icp.icp(Sd, Td, [torch.eye(4, dtype=dtype, device=DEV)] * N, **kw)
    out["T"].sum().backward()
    assert float((out["T"].cpu() - ref["T"]).abs().max()) < 1e-9
    for b in range(N):
        assert float((Sd[b].grad.cpu() - sc.grad[b, :SRC_ROWS[b]]).abs().max()) < 1e-8
        assert float((Td[b].grad.cpu() - tc.grad[b, :TGT_ROWS[b]]).abs().max()) < 1e-8
