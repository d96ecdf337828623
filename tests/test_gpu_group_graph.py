"""The operators of dicp_amd.group inside a captured graph (torch.cuda.graph) on the MI355X.

Forward + backward of pool_neighbors (each reduce), group_points (with centers) and interpolate_features are captured once on static device
tensors with device rows -- a linear chain of kernels, no parallel branches -- after a warm-up on a side stream, and replayed twice with
different data copied into the static inputs, each replay followed by a synchronisation (the zero fill of the gradient table must be
ordered like a kernel: csrc/dicp_fill.h).  Every replay is compared with eager calls on the same data: the forward outputs, argmax,
counts, g_centers and g_d2 bit for bit; g_features, which is added with float atomics in an order that differs from run to run, within
(D + k + 8) u sum|terms| of the float64 sum of its terms -- the eager run and the replay alike, D the row's in-degree."""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.group import group_points, interpolate_features, pool_neighbors

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_ref as gr  # noqa: E402

pytestmark = pytest.mark.gpu

N, N_Q, M_ROWS, K = 2, 63, 257, 8
ROWS = [M_ROWS * 3 // 4, M_ROWS]
EPS = 1e-8
U = float(np.finfo(np.float32).eps) / 2


def _data(C, seed):
    """one set of inputs on the device: features, idx, d2, centres, the cotangents of a (N, n, C) and of a (N, n, k, C) output"""
    rng = np.random.default_rng(seed)

    def table(shape):
        return torch.from_numpy(((rng.random(shape) * 2 - 1) * 10.0 ** rng.integers(-2, 3, size=shape)).astype(np.float32)).cuda()
    idx = torch.from_numpy(np.stack([gr.make_idx(N_Q, K, M_ROWS, ROWS[b], seed + 10 + b) for b in range(N)])).cuda()
    d2 = torch.from_numpy(np.stack([gr.make_d2(N_Q, K, seed + 20 + b, np.float32, near=True) for b in range(N)])).cuda()
    return {"f": table((N, M_ROWS, C)), "idx": idx, "d2": d2, "cen": table((N, N_Q, 3)), "g": table((N, N_Q, C)), "g4": table((N, N_Q, K, C))}


def _op(name):
    """-> fn(inputs, rows) -> (outputs compared bit for bit, g_features)"""
    def pool(reduce):
        def run(x, rows):
            f = x["f"].detach().requires_grad_(True)
            res = pool_neighbors(f, x["idx"], reduce, rows=rows, return_argmax=reduce == "max", return_counts=True)    # out, (argmax,) counts
            gf, = torch.autograd.grad(res[0], [f], x["g"])
            return [res[0].detach(), res[-1]] + list(res[1:-1]), gf
        return run

    def group(x, rows):
        f, cen = x["f"].detach().requires_grad_(True), x["cen"].detach().requires_grad_(True)
        out = group_points(f, x["idx"], rows=rows, centers=cen)
        gf, gc = torch.autograd.grad(out, [f, cen], x["g4"])
        return [out.detach(), gc], gf

    def interp(x, rows):
        f, d2 = x["f"].detach().requires_grad_(True), x["d2"].detach().requires_grad_(True)
        out = interpolate_features(f, x["idx"], d2, eps=EPS, rows=rows)
        gf, gd = torch.autograd.grad(out, [f, d2], x["g"])
        return [out.detach(), gd], gf
    return {"pool_max": pool("max"), "pool_mean": pool("mean"), "pool_sum": pool("sum"), "group_points": group, "interpolate_features": interp}[name]


def _exact_gf(name, x, rows, arg):
    """float64: g_features as the sum of its terms, the sum of their magnitudes, and the in-degree of every row -- a torch graph on the
    same indices (clamp, gather, mask); the maximum's through the argmax the eager call returned"""
    f = x["f"].double().requires_grad_(True)
    idx = x["idx"]
    live = (idx >= 0) & (idx < rows.view(-1, 1, 1))
    safe = idx.clamp(min=0, max=M_ROWS - 1)
    bi = torch.arange(N, device="cuda")[:, None, None]
    zero = torch.zeros((), dtype=torch.float64, device="cuda")
    gathered = torch.where(live[..., None], f[bi, safe], zero)                                     # (N, n, k, C)
    g = x["g"].double()
    if name == "group_points":
        out, g = gathered, x["g4"].double()
    elif name == "pool_sum":
        out = gathered.sum(2)
    elif name == "pool_mean":
        out = gathered.sum(2) / live.sum(2, keepdim=True).clamp(min=1)
    elif name == "pool_max":
        out = torch.where(arg >= 0, f[bi, arg.clamp(min=0).long(), torch.arange(f.shape[2], device="cuda")], zero)
    else:
        r = torch.where(live, 1.0 / (x["d2"].double() + float(np.float32(EPS))), zero)
        out = ((r / r.sum(2, keepdim=True).clamp(min=1e-300))[..., None] * gathered).sum(2)
    ref, = torch.autograd.grad(out, [f], g, retain_graph=True)
    mag, = torch.autograd.grad(out, [f], g.abs())                                                 # (every term's weight is >= 0)
    deg = torch.zeros(N * M_ROWS, dtype=torch.float64, device="cuda").index_add_(0, (safe + bi * M_ROWS).reshape(-1), live.reshape(-1).double())
    return ref, mag, deg.view(N, M_ROWS, 1)


@pytest.mark.parametrize("C", [3, 64])
@pytest.mark.parametrize("name", ["pool_max", "pool_mean", "pool_sum", "group_points", "interpolate_features"])
def test_captured_forward_and_backward(name, C):
    run = _op(name)
    static = _data(C, 1)
    rows = torch.tensor(ROWS, dtype=torch.int32).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run(static, rows)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        exact_g, gf_g = run(static, rows)
    for seed in (2, 3):
        fresh = _data(C, seed)
        for key, t in fresh.items():
            static[key].copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        exact_e, gf_e = run(fresh, rows)
        assert len(exact_e) == len(exact_g)
        for a, b in zip(exact_g, exact_e):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, seed)      # bit for bit
        arg = exact_e[2] if name == "pool_max" else None
        ref, mag, deg = _exact_gf(name, fresh, rows, arg)
        bound = (deg + K + 8) * U * mag
        for got in (gf_g, gf_e):
            assert torch.isfinite(got).all() and (got != 0).any()
            assert ((got.double() - ref).abs() <= bound).all(), (name, seed)
            assert (got[(deg == 0).expand_as(got)] == 0).all()
