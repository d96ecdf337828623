"""estimate_normals(method="grid") without a GPU: the argument check; the new entry points' refusals; the self-query form of the grid scan
(the header the kernel runs, built for the host: gridknn_host.header(P, P, k)) against the brute force on the clouds that
tests/test_gpu_normals_grid.py puts on the GPU, so that every expected neighbour list there is proved here as well -- duplicates, the
lattice's ties across cells and non-finite rows included; and the numpy model of the backward window in grid order (normals_grid_model),
with the conditions of the gradient layouts asserted before any GPU result is looked at."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import _lib
from dicp_amd.normals import estimate_normals

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ball_clouds as bc  # noqa: E402
import gridknn_host as gh  # noqa: E402
import normals_grid_model as ng  # noqa: E402
import walk_layouts as wl  # noqa: E402
from test_gpu_normals import SMALL, _cloud  # noqa: E402  (the small clouds of the walk's tests, as the GPU file takes them)

DTYPES = [np.float32, np.float64]


# ------------------------------------------------------------------ the argument check
@pytest.mark.parametrize("method", ["octree", None, 1, "Grid", b"grid"])
def test_another_method_is_a_value_error(method):
    pts = torch.zeros((10, 3))
    with pytest.raises(ValueError, match='estimate_normals: method must be "walk" or "grid"'):
        estimate_normals(pts, method=method)


def test_method_is_the_last_public_keyword():
    import inspect
    names = list(inspect.signature(estimate_normals).parameters)
    assert names[:7] == ["points", "k", "viewpoint", "rows", "return_curvature", "return_neighbors", "method"]
    assert inspect.signature(estimate_normals).parameters["method"].default == "walk"


def test_grid_entry_points_reject_bad_arguments():
    """null pointers, bad shapes, dtypes and alignment are refused before any launch (no GPU is touched)"""
    _lib.build()
    lib = _lib.load()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)
    big = 1 << 40
    assert lib.dicp_normals_grid_workspace_bytes(0, 2, 1000, 16, 3, 0) >= 2 * 1024 * (8 + 4 + 16 + 16 * 4) + 2 * 128
    assert lib.dicp_normals_grid_workspace_bytes(1, 2, 1000, 16, 3, 1) >= 2 * 1024 * 3 * 8
    for bad in ((7, 2, 1000, 16, 3), (0, 0, 1000, 16, 3), (0, 2, 0, 16, 3), (0, 2, 1000, 2, 3), (0, 2, 1000, 33, 3), (0, 2, 1000, 16, 2),
                (0, 2, (1 << 30) + 1, 16, 3)):
        assert lib.dicp_normals_grid_workspace_bytes(*bad, 0) == 0 and lib.dicp_normals_grid_workspace_bytes(*bad, 1) == 0, bad

    def fwd(dtype=0, pts=one, c=3, rows=None, N=1, m=10, k=8, vp=None, per=0, nrm=one, curv=None, nbr=None, ws=one, wsb=big, vis=None, pas=None):
        return lib.dicp_normals_grid_forward(dtype, pts, c, rows, N, m, k, vp, per, nrm, curv, nbr, ws, wsb, vis, pas, None)
    assert fwd(pts=None) == 1 and fwd(nrm=None) == 1 and fwd(ws=None) == 1
    assert fwd(dtype=5) == 3
    assert fwd(c=2) == 2 and fwd(k=2) == 2 and fwd(k=33) == 2 and fwd(m=0) == 2 and fwd(N=0) == 2 and fwd(per=2) == 2 and fwd(wsb=64) == 2
    assert fwd(ws=odd) == 5 and fwd(pts=ctypes.c_void_p(258)) == 5 and fwd(nbr=odd) == 5 and fwd(vis=odd) == 5 and fwd(pas=odd) == 5
    assert fwd(rows=ctypes.c_void_p(258)) == 5 and fwd(dtype=1, curv=odd) == 5 and fwd(dtype=1, vp=odd) == 5

    def bwd(dtype=0, gn=one, gc=None, vp=None, per=0, N=1, m=10, k=8, c=3, fws=one, grad=one, ws=one, wsb=big):
        return lib.dicp_normals_grid_backward(dtype, gn, gc, vp, per, N, m, k, c, fws, grad, ws, wsb, None)
    assert bwd(fws=None) == 1 and bwd(grad=None) == 1 and bwd(ws=None) == 1
    assert bwd(dtype=2) == 3
    assert bwd(c=2) == 2 and bwd(k=40) == 2 and bwd(m=-1) == 2 and bwd(per=3) == 2 and bwd(wsb=8) == 2
    assert bwd(fws=odd) == 5 and bwd(ws=odd) == 5 and bwd(dtype=1, grad=odd) == 5 and bwd(dtype=1, gn=odd) == 5 and bwd(dtype=1, gc=odd) == 5


# ------------------------------------------------------------------ the self-query scan against the brute force
def _hold_self(P, k, rows=None):
    got, st = gh.header(P, P, k, x_rows=rows, y_rows=rows)
    bad = gh.same(got, gh.reference(P, P, k, x_rows=rows, y_rows=rows))
    assert bad is None, bad
    return got, st


@pytest.mark.parametrize("m,k,dtype", SMALL)
def test_self_query_small_clouds(m, k, dtype):
    pts = _cloud(3, m, dtype, seed=m * 100 + k).numpy()
    for b in range(3):
        (_, idx), _ = _hold_self(pts[b], k)
        assert (idx[:, 0] == np.arange(m)).all()            # random rows: every row is its own nearest


@pytest.mark.parametrize("dtype", DTYPES)
def test_self_query_grid_layouts(dtype):
    """the y cloud of every layout of the grid k-NN tests and of the non-finite pair, at the k of the GPU test"""
    names = set()
    for name, _, y in gh.all_cases(dtype) + [("non-finite rows", None, bc.nonfinite_pair(dtype)[1])]:
        names.add(name)
        for k in (8, 32):
            (d2, idx), _ = _hold_self(y, k)
            if name == "300 copies":
                assert (idx == np.arange(k)[None, :]).all() and (d2 == 0).all()      # 300 rows at d2 = 0: the lowest indices, for every row
            if name == "lattice r=1.0" and k == 8:
                assert idx[171, :7].tolist() == [171, 122, 164, 170, 172, 178, 220]  # six rows at d2 = 1 in six cells: by index
            if name == "non-finite rows":
                assert (idx[[5, 17, 400, 899]] == -1).all() and not np.isin(idx, [5, 17, 400, 899]).any()
            if name == "extent 3e38" and dtype == np.float32:
                assert ((idx >= 0).sum(1) == [1, 1, 2, 2]).all()                     # the other d2 overflow: no candidates
    assert {"300 copies", "line along z", "line along x", "wall", "two clusters", "extent 3e38", "non-finite rows"} <= names


def test_self_query_large_and_ragged_clouds():
    P = _cloud(1, 20000, torch.float32, seed=20016, scale=10.0)[0].numpy()
    _hold_self(P, 16)
    for dtype in (torch.float32, torch.float64):
        pts = _cloud(4, 1000, dtype, seed=1011).numpy()
        for b, r in enumerate([1000, 6, 0, 333]):
            _hold_self(pts[b], 8, rows=r)


# ------------------------------------------------------------------ the grid's order and the backward window in it
@pytest.mark.parametrize("dtype", DTYPES)
def test_grid_order_model(dtype):
    """live rows first, by (key, index); the rows that stay out after them, by index; equal keys are whole cells"""
    P = bc.nonfinite_pair(dtype)[1]
    g = ng.grid_order(P, rows=850)
    out = sorted([5, 17, 400] + list(range(850, 900)))
    assert g.cnt == 847 and not g.flat and g.perm[g.cnt:].tolist() == out
    ks = g.keys[g.perm[:g.cnt]]
    assert (ks[1:] >= ks[:-1]).all() and (ks != ng.NO_KEY).all()
    same = ks[1:] == ks[:-1]
    assert same.any() and (g.perm[1:g.cnt][same] > g.perm[:g.cnt - 1][same]).all()
    assert 0.5 <= g.cnt / np.unique(ks).size <= 8.0         # about two rows per cell of the box
    w = ng.grid_order(wl.wall(6000, 0).astype(dtype))
    assert w.hi[0] == 0 and w.hi[1] > 8 and w.hi[2] > 8     # one cell in x


@pytest.mark.parametrize("name,dtype", ng.GRAD_LAYOUTS)
def test_gradient_layouts_meet_their_conditions(name, dtype):
    """cube(40000) float32 and cube(20000) float64 put at least 0.2 of the backward's entries outside the window and 0.2 inside;
    wall(6000) puts none outside.  (The lists are the float64 model's here; the GPU test repeats this on the brute force's.)"""
    P = ng.grad_layout(name, dtype)
    nbr = wl.model_neighbours(P, P, ng.K_GRAD)
    s = ng.check_grad_conditions(name, ng.grid_windows(P, ng.K_GRAD, dtype, nbr))
    print("normals grid %s %s: backward entries outside the window %.3f" % (name, dtype, s))
    walk = wl.normals_windows(P, ng.K_GRAD, dtype, nbr).share()
    print("normals walk %s %s: %.3f" % (name, dtype, walk))
    if name == "wall":
        assert walk > 0.5                                   # the same wall leaves the x-sorted window: the two orders differ
