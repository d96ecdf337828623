"""CPU checks of the surface-normal estimate (dicp_amd/normals.py) that need no GPU.

``dicp_amd/csrc/dicp_normals.h`` -- the per-point arithmetic of the HIP kernels -- is compiled with g++ through
tests/hostcheck/normals_check.cpp and held to numpy's eigh (forward) and to torch autograd through torch.linalg.eigh
(backward); the argument checks of ``estimate_normals`` run before any device work.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.normals import estimate_normals

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostbuild  # noqa: E402


@pytest.fixture(scope="module")
def nc():
    lib = hostbuild.build("normals_check.cpp", "normals_check")
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.nc_forward.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.nc_forward.restype = None
    lib.nc_backward.argtypes = [vp, i32, vp, vp, f64, f64, vp]
    lib.nc_backward.restype = i32
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _forward(nc, q, dv):
    q = np.ascontiguousarray(q, dtype=np.float64)
    dv = np.ascontiguousarray(dv, dtype=np.float64)
    n, curv, lam, v = np.zeros(3), np.zeros(1), np.zeros(3), np.zeros(9)
    nc.nc_forward(_p(q), q.shape[0], _p(dv), _p(n), _p(curv), _p(lam), _p(v))
    return n, curv[0], lam, v.reshape(3, 3)


def _backward(nc, q, dv, gn, gk, tau=1e-12):
    q = np.ascontiguousarray(q, dtype=np.float64)
    dv = np.ascontiguousarray(dv, dtype=np.float64)
    gn = np.ascontiguousarray(gn, dtype=np.float64)
    gq = np.zeros_like(q)
    on = nc.nc_backward(_p(q), q.shape[0], _p(dv), _p(gn), float(gk), tau, _p(gq))
    return gq, on


def _neighbourhood(rng, k, scales):
    """k points of an anisotropic cloud, the first one the query point; -> (points (k,3), offsets q = p - p_0)"""
    R, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    pts = (rng.standard_normal((k, 3)) * scales) @ R.T + rng.standard_normal(3) * 5.0
    return pts, pts - pts[0]


def _oracle(q):
    mu = q.mean(0)
    C = (q - mu).T @ (q - mu) / q.shape[0]
    w, V = np.linalg.eigh(C)
    return w, V


def test_forward_matches_eigh(nc):
    rng = np.random.default_rng(3)
    for t in range(200):
        k = int(rng.integers(3, 33))
        scales = np.sort(rng.uniform(0.01, 2.0, 3))[::-1]
        pts, q = _neighbourhood(rng, k, scales)
        dv = rng.standard_normal(3) * 10.0
        n, curv, lam, v = _forward(nc, q, dv)
        w, V = _oracle(q)
        np.testing.assert_allclose(lam, w, rtol=1e-9, atol=1e-12 * w[2])
        assert abs(np.linalg.norm(n) - 1.0) < 1e-12
        if (w[1] - w[0]) > 1e-6 * w.sum():
            assert abs(abs(n @ V[:, 0]) - 1.0) < 1e-10
        assert n @ dv >= 0
        np.testing.assert_allclose(curv, w[0] / w.sum(), rtol=1e-9, atol=1e-15)


def test_orientation_on_a_zero_dot_product(nc):
    q = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [-1, 0, 0], [0, -2, 0], [0.5, 0.5, 0]], dtype=np.float64)
    n, _, _, _ = _forward(nc, q, np.array([3.0, -1.0, 0.0]))       # the plane z = 0 seen from inside it
    np.testing.assert_allclose(n, [0, 0, 1], atol=1e-12)
    n2, _, _, _ = _forward(nc, q, np.array([0.0, 0.0, -2.0]))
    np.testing.assert_allclose(n2, [0, 0, -1], atol=1e-12)


def _autograd(pts, gn, gk, n_fwd):
    """dL/dp of L = gn . n + gk curvature through torch.linalg.eigh, its eigenvector signed like the forward's normal n_fwd"""
    p = torch.tensor(pts, dtype=torch.float64, requires_grad=True)
    q = p - p[0]
    mu = q.mean(0)
    C = (q - mu).T @ (q - mu) / q.shape[0]
    w, V = torch.linalg.eigh(C)
    sign = 1.0 if float(V[:, 0].detach().numpy() @ n_fwd) > 0 else -1.0
    n = sign * V[:, 0]
    L = (n * torch.tensor(gn)).sum() + gk * w[0] / w.sum()
    L.backward()
    return p.grad.numpy()


def test_backward_matches_autograd(nc):
    rng = np.random.default_rng(5)
    for t in range(100):
        k = int(rng.integers(3, 33))
        scales = np.array([2.0, 1.0, 0.2]) * rng.uniform(0.5, 2.0)
        pts, q = _neighbourhood(rng, k, scales)
        w, V = _oracle(q)
        if w[1] - w[0] < 0.05 * w.sum() or w[2] - w[1] < 0.05 * w.sum():
            continue
        dv = rng.standard_normal(3) * 10.0
        gn = rng.standard_normal(3)
        gk = float(rng.standard_normal()) if t % 2 else 0.0
        n, _, _, _ = _forward(nc, q, dv)
        gq, on = _backward(nc, q, dv, gn, gk)
        assert on == 1
        ref = _autograd(pts, gn, gk, n)
        np.testing.assert_allclose(gq, ref, rtol=1e-8, atol=1e-10 * np.abs(ref).max())


@pytest.mark.parametrize("kind", ["collinear", "coincident"])
def test_degenerate_neighbourhoods(nc, kind):
    rng = np.random.default_rng(7)
    k = 12
    if kind == "collinear":
        d = rng.standard_normal(3)
        q = np.outer(rng.standard_normal(k), d / np.linalg.norm(d))
        q -= q[0]
    else:
        q = np.zeros((k, 3))
    n, curv, lam, _ = _forward(nc, q, np.array([1.0, 2.0, 3.0]))
    assert np.all(np.isfinite(n)) and np.isfinite(curv)
    assert abs(np.linalg.norm(n) - 1.0) < 1e-12
    if kind == "collinear":
        assert abs(n @ (d / np.linalg.norm(d))) < 1e-8
    else:
        assert curv == 0.0
    gq, on = _backward(nc, q, np.array([1.0, 2.0, 3.0]), rng.standard_normal(3), 0.7)
    assert on == 0
    assert np.all(gq == 0.0)


@pytest.mark.parametrize("k", [0, 2, 33])
def test_bad_k_raises(k):
    with pytest.raises(ValueError):
        estimate_normals(torch.zeros(10, 3), k=k)


def test_two_columns_raise():
    with pytest.raises(ValueError):
        estimate_normals(torch.zeros(10, 2), k=8)
    with pytest.raises(ValueError):
        estimate_normals([torch.zeros(10, 3), torch.zeros(5, 2)], k=8)


def test_integer_dtype_raises():
    with pytest.raises(ValueError):
        estimate_normals(torch.zeros(10, 3, dtype=torch.int64), k=8)
    with pytest.raises(ValueError):
        estimate_normals(torch.zeros(10, 3, dtype=torch.int32), k=8)


def test_other_arguments_raise():
    with pytest.raises(ValueError):
        estimate_normals(torch.zeros(2, 10, 3), k=8, rows=[3])
    with pytest.raises(ValueError):
        estimate_normals(torch.zeros(2, 10, 3), k=8, rows=[3, 11])
    with pytest.raises(ValueError):
        estimate_normals(torch.zeros(2, 10, 3), k=8, viewpoint=torch.zeros(3, 3))
    with pytest.raises(ValueError):
        estimate_normals(torch.zeros(4, 10, 3, 1), k=8)
