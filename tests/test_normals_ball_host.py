"""CPU checks of the whole-ball normals (dicp_amd/normals.py: estimate_normals_ball) that need no GPU.

``dicp_amd/csrc/dicp_normals_ball.h`` -- the forward, the records and the gather the HIP kernels execute -- is compiled with g++ through
tests/hostcheck/normals_ball_check.cpp, run on a host-sorted grid and held to tests/normals_ball_ref.py BIT FOR BIT in float32 and
float64: counts, eigenvalues, normals, curvature, and, given records, the gradient.  The eigenvalues are also held to tests/iss_ref.py's
(the ISS pass's) bit for bit.  The records are held to torch autograd on a float64 composition (constant membership mask, masked mean and
covariance, torch.linalg.eigh, the reference's sign) within the project's gradcheck tolerances.  The symmetry claim of the header -- j is
a member of i exactly when i is a member of j -- is asserted on every layout.  The comparison is shown to refuse a gather in row order.
The conditions of the GPU tests' designed cases (the wavy sheet, the cluster lattice) are asserted here on the references alone.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostbuild  # noqa: E402
import iss_ball_cases as ibc  # noqa: E402
import iss_ball_ref as ibr  # noqa: E402
import iss_ref as ir  # noqa: E402
import normals_ball_cases as nbc  # noqa: E402
import normals_ball_ref as nbr  # noqa: E402

RIGHT, ROW_ORDER = 0, 1
DTYPES = [np.float32, np.float64]
STATE = 11
ATOL, RTOL = 1e-6, 1e-4                                     # the project's gradcheck tolerances


@pytest.fixture(scope="module")
def lib():
    so = hostbuild.build("normals_ball_check.cpp", "normals_ball_check")
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    so.nbc_forward.argtypes, so.nbc_forward.restype = [i32, vp, i32, i32, i32, f64, vp, i32, vp, vp, vp, vp, vp, vp, vp], None
    so.nbc_records.argtypes, so.nbc_records.restype = [i32, vp, i32, i32, vp, vp, vp, vp, vp], None
    so.nbc_gather.argtypes, so.nbc_gather.restype = [i32, vp, i32, i32, i32, f64, vp, i32, vp, vp], None
    so.nbc_eigen.argtypes, so.nbc_eigen.restype = [i32, vp, vp, vp, vp], None
    so.nbc_sign.argtypes, so.nbc_sign.restype = [i32, vp, vp, vp], None
    return so


@pytest.fixture(scope="module")
def plan_lib():
    so = hostbuild.build("iss_ball_check.cpp", "iss_ball_check")
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    so.ibc_plan.argtypes, so.ibc_plan.restype = [i32, vp, i32, i32, i32, f64, vp, vp], None
    return so


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_plan(plan_lib, pts, rows, radius):
    """the host build's plan of one cloud (tests/test_iss_ball_host.py's) -> None where the simple rule stands, else (edges, enlarged, flat)"""
    pts = np.ascontiguousarray(pts)
    edges, flags = np.zeros(3), np.zeros(3, np.int32)
    plan_lib.ibc_plan(int(pts.dtype == np.float64), _p(pts), pts.shape[1], pts.shape[0], pts.shape[0] if rows is None else rows, float(radius),
                      _p(edges), _p(flags))
    return (edges.astype(pts.dtype), bool(flags[0]), bool(flags[1])) if (flags[0] or flags[1]) else None


def host_forward(lib, pts, radius, rows=None, viewpoint=None, min_neighbors=3):
    pts = np.ascontiguousarray(pts)
    m, dt = pts.shape[0], pts.dtype
    nrm, curv, eig = np.zeros((m, 3), dt), np.zeros(m, dt), np.zeros((m, 3), dt)
    cnt, order, state, stats = np.zeros(m, np.int32), np.zeros(m, np.int64), np.zeros((m, STATE)), np.zeros(4, np.int64)
    vp = None if viewpoint is None else np.ascontiguousarray(np.asarray(viewpoint, dtype=dt).astype(np.float64))
    lib.nbc_forward(int(dt == np.float64), _p(pts), pts.shape[1], m, m if rows is None else rows, float(radius), _p(vp), min_neighbors,
                    _p(nrm), _p(curv), _p(eig), _p(cnt), _p(order), _p(state), _p(stats))
    return dict(normals=nrm, curv=curv, eig=eig, count=cnt, order=order[order >= 0], state=state, stats=stats)


def host_records(lib, pts, fwd, gn, gk):
    pts = np.ascontiguousarray(pts)
    m = pts.shape[0]
    rec = np.zeros((m, nbr.REC))
    live = np.ascontiguousarray((fwd["count"] > 0).astype(np.uint8))
    gn = None if gn is None else np.ascontiguousarray(gn, dtype=pts.dtype)
    gk = None if gk is None else np.ascontiguousarray(gk, dtype=pts.dtype)
    lib.nbc_records(int(pts.dtype == np.float64), _p(pts), pts.shape[1], m, _p(fwd["state"]), _p(live), _p(gn), _p(gk), _p(rec))
    return rec


def host_gather(lib, pts, radius, rec, rows=None, variant=RIGHT):
    pts = np.ascontiguousarray(pts)
    m = pts.shape[0]
    grad, stats = np.zeros((m, 3), pts.dtype), np.zeros(1, np.int64)
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    lib.nbc_gather(int(pts.dtype == np.float64), _p(pts), pts.shape[1], m, m if rows is None else rows, float(radius), _p(rec), variant, _p(grad),
                   _p(stats))
    return grad, int(stats[0])


def cotangents(seed, m, dtype):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((m, 3)).astype(dtype), rng.standard_normal(m).astype(dtype)


def check_cloud(lib, plan_lib, P, radius, rows=None, viewpoint=None, min_neighbors=3, seed=0):
    """forward and, on the header's own records, the gather of one cloud against the reference, bit for bit -> (reference, records)"""
    plan = host_plan(plan_lib, P, rows, radius)
    want = nbr.forward_ref(P, radius, rows, viewpoint, min_neighbors, plan)
    got = host_forward(lib, P, radius, rows, viewpoint, min_neighbors)
    assert ir.same_bits(got["order"], want["order"])
    for key in ("count", "eig", "normals", "curv"):
        assert ir.same_bits(got[key], want[key]), key
    iss = ibr.keypoints_ball_ref(P, radius, None, rows, plan=plan)
    assert ir.same_bits(got["eig"], iss["eig"]) and ir.same_bits(got["count"], iss["count"])          # the ISS pass's, bit for bit
    on = want["count"] >= min_neighbors
    assert np.allclose(np.linalg.norm(want["n64"][on], axis=1), 1.0, rtol=0, atol=1e-12)
    assert not want["normals"][~on].any() and not want["curv"][~on].any()
    gn, gk = cotangents(seed, P.shape[0], P.dtype)
    rec = host_records(lib, P, got, gn, gk)
    assert not rec[~on][:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 12]].any()                                      # f = 0 with G = mu = 0
    grad, visited = host_gather(lib, P, radius, rec, rows)
    assert ir.same_bits(grad, nbr.gather_ref(P, rec, radius, rows, plan))
    assert visited * 2 == got["stats"][0]                                                              # one walk against the forward's two
    assert not grad[want["count"] == 0].any()
    return want, rec


# ------------------------------------------------------------------ the eigen-system alone
def test_eigen_system_and_sign(lib):
    rng = np.random.default_rng(3)
    B = rng.standard_normal((400, 5, 3)) * np.array([1.0, 0.3, 0.02])
    B[:50] *= 1e-4
    B[50:60, :, 2] = 0.0                                                            # planar: a zero eigenvalue
    B[60:70, :, 1:] = 0.0                                                           # collinear
    C = np.einsum("nka,nkb->nab", B, B) / 5.0
    C[70] = np.diag([3.0, 1.0, 1.0])                                                # already diagonal, a tie: the lower index first
    C[71] = 0.0
    a = np.ascontiguousarray(np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], axis=-1))
    n = a.shape[0]
    lam, v, iss_lam = np.zeros((n, 3)), np.zeros((n, 9)), np.zeros((n, 3))
    lib.nbc_eigen(n, _p(a), _p(lam), _p(v), _p(iss_lam))
    assert ir.same_bits(lam, iss_lam) and ir.same_bits(lam, ir.eigenvalues(list(a.T)))
    want_lam, want_v = nbr.eigen(list(a.T))
    assert ir.same_bits(lam, want_lam) and ir.same_bits(v.reshape(n, 3, 3), want_v)
    V = v.reshape(n, 3, 3)                                                          # V[:, k] the k-th eigenvector
    assert np.array_equal(V[70], np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]])) and np.array_equal(V[71], np.eye(3))
    scale = np.abs(lam).max(axis=1)[:, None, None] + 1e-300
    assert np.abs(np.einsum("nab,nkb->nka", C, V) - lam[:, :, None] * V).max() < 1e-13 * scale.max()
    assert (np.abs(np.einsum("nab,nkb->nka", C, V) - lam[:, :, None] * V) <= 64 * 2.0 ** -53 * scale).all()
    assert np.abs(np.einsum("nka,nla->nkl", V, V) - np.eye(3)).max() < 1e-14
    # the sign rule, a dot product of exactly 0 included
    v0 = np.array([[0.0, -1.0, 0.0], [1.0, 1.0, 0.0], [-1.0, -1.0, 0.0], [0.0, 0.0, -0.5], [0.0, 0.0, 0.0], [0.3, 0.2, 0.1], [0.3, 0.2, 0.1]])
    d = np.array([[1.0, 0.0, 0.0], [1.0, -1.0, 0.0], [1.0, -1.0, 5.0], [1.0, 1.0, 0.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]])
    s = np.zeros(len(v0))
    lib.nbc_sign(len(v0), _p(v0), _p(d), _p(s))
    assert list(s) == [-1.0, 1.0, -1.0, -1.0, 1.0, 1.0, -1.0] and np.array_equal(s, nbr.sign(v0, d))


# ------------------------------------------------------------------ the header against the reference
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,rows,members,cols", [(300, None, 12, 3), (300, 211, 40, 4), (65, None, 12, 3), (65, 50, 6, 6), (40, 33, 8, 3),
                                                 (40, None, 8, 3), (2, None, 1, 3), (2, 1, 1, 3), (1, None, 1, 3)])
def test_random_clouds(lib, plan_lib, dtype, m, rows, members, cols):
    P = np.full((m, cols), np.nan, dtype=dtype)
    P[:, :3] = ibc.cube(m + members, m, dtype)
    if m >= 40:
        P[3, 1], P[9, 0], P[11] = np.nan, np.inf, P[10]                             # a NaN row, an inf row, an exact duplicate
    radius = ibc.ball_radius(P[:rows], members) if m > 2 else 0.5
    for vp, min_nb in ((None, 3), ([0.3, -2.0, 5.0], 5)):
        want, _ = check_cloud(lib, plan_lib, P, radius, rows, vp, min_nb, seed=m)
    if m >= 40:
        assert not want["count"][3] and not want["count"][9] and want["count"][10] == want["count"][11]
        assert ((want["count"] > 0) & (want["count"] < 5)).any() or members > 8      # (sparse balls: rows below min_neighbors = 5 exist)
        assert (want["count"] >= 5).sum() > m // 3
    if rows is not None:
        assert not want["count"][rows:].any() and not want["normals"][rows:].any()
    if m <= 2:
        assert not want["normals"].any() and want["count"].max() <= 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["planar", "collinear", "only_itself", "non_finite"])
def test_designed_clouds(lib, plan_lib, dtype, name):
    P, rows, r, _ = ibc.designed(dtype)[name]
    want, rec = check_cloud(lib, plan_lib, P, r, rows, [0.0, 0.0, 10.0])
    if name == "planar":
        assert (want["eig"][:, 0] == 0).all() and (want["curv"] == 0).all() and (np.abs(want["normals"][:, 2]) == 1).all()
        inplane, _ = check_cloud(lib, plan_lib, P, r, rows, [7.0, 3.0, float(P[0, 2])])               # d_z = 0: the dot product is exactly 0
        assert (np.abs(inplane["normals"][:, 2]) == 1).all()
    if name == "collinear":
        assert not want["eig"][:, :2].any() and not rec[:, 12].any()                 # lam_0 = lam_1: no gradient
    if name == "only_itself":
        assert list(want["count"]) == [1, 1, 0, 0, 0, 0] and not want["normals"].any() and not rec[:, 12].any()
    if name == "non_finite":
        assert list(want["count"]) == [9] * 9 + [0, 0] and (np.abs(np.linalg.norm(want["n64"][:9], axis=1) - 1) < 1e-12).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ibc.LAYOUT_NAMES)
def test_layouts(lib, plan_lib, dtype, name):
    """the layouts of the coverage claim (rows exactly at R, a radius that rounds down, enlarged edges, a flat grid), with the symmetry
    claim: the brute-force membership matrix is symmetric"""
    P, r, _ = ibc.layouts(dtype)[name]
    plan = host_plan(plan_lib, P, None, r)
    assert (plan is not None) == (name in ("two clusters", "far outlier", "flat")) and (plan is None or plan[2] == (name == "flat"))
    want, _ = check_cloud(lib, plan_lib, P, r)
    brute = ibr.members_brute(P, None, r)
    assert np.array_equal(brute, brute.T) and brute.sum() > 0
    assert np.array_equal(want["count"], np.where(np.isfinite(P).all(-1), 1 + brute.sum(axis=1), 0))


@pytest.mark.parametrize("dtype", DTYPES)
def test_membership_is_symmetric(dtype):
    for seed, m, members in ((1, 300, 12), (2, 300, 40), (3, 65, 6)):
        P = ibc.cube(seed, m, dtype)
        P[11] = P[10]
        for r in (ibc.ball_radius(P, members), float(np.linalg.norm(P[0].astype(np.float64) - P[1].astype(np.float64)))):
            brute = ibr.members_brute(P, None, r)
            assert np.array_equal(brute, brute.T) and brute[10, 11]
    for name in ("planar", "collinear", "only_itself", "non_finite"):
        P, rows, r, _ = ibc.designed(dtype)[name]
        brute = ibr.members_brute(P, rows, r)
        assert np.array_equal(brute, brute.T)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_cloud_with_no_live_rows(lib, plan_lib, dtype):
    P = ibc.cube(1, 12, dtype)
    want, rec = check_cloud(lib, plan_lib, P, 0.5, rows=0)
    assert not want["count"].any() and not want["eig"].any() and not want["normals"].any() and not rec[:, 12].any()


# ------------------------------------------------------------------ the gather refuses a wrong order; absent and zero cotangents
def test_refuses_a_gather_in_row_order(lib, plan_lib):
    """(float64: rounded to float32 the two orders give the same gradient on almost every row)"""
    P = ibc.cube(5, 300, np.float64)
    r = ibc.ball_radius(P, 40)
    fwd = host_forward(lib, P, r)
    rec = host_records(lib, P, fwd, *cotangents(9, 300, np.float64))
    right, wrong = nbr.gather_ref(P, rec, r), nbr.gather_ref(P, rec, r, row_order=True)
    assert ir.same_bits(host_gather(lib, P, r, rec)[0], right)
    assert not ir.same_bits(wrong, right) and np.allclose(wrong, right, rtol=1e-9, atol=1e-13)
    got = host_gather(lib, P, r, rec, variant=ROW_ORDER)[0]
    assert ir.same_bits(got, wrong) and not ir.same_bits(got, right)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cotangents_absent_or_zero(lib, dtype):
    P = ibc.cube(7, 65, dtype)
    r = ibc.ball_radius(P, 10)
    fwd = host_forward(lib, P, r)
    gn, gk = cotangents(2, 65, dtype)
    zero_n, zero_k = np.zeros_like(gn), np.zeros_like(gk)
    for a, b in ((None, None), (zero_n, None), (None, zero_k), (zero_n, zero_k), (-zero_n, -zero_k)):
        rec = host_records(lib, P, fwd, a, b)
        assert not rec[:, :9].any() and not rec[:, 12].any()
        assert not host_gather(lib, P, r, rec)[0].any()
    both, only_n, only_k = (host_records(lib, P, fwd, a, b) for a, b in ((gn, gk), (gn, None), (None, gk)))
    assert np.allclose(both[:, :6], only_n[:, :6] + only_k[:, :6], rtol=1e-12, atol=1e-300) 
    on = fwd["count"] >= 3
    assert on.sum() > 50 and np.array_equal(only_n[:, 12] != 0, on) and np.array_equal(only_k[:, 12] != 0, on)
    assert ir.same_bits(host_records(lib, P, fwd, gn, zero_k), only_n) and ir.same_bits(host_records(lib, P, fwd, zero_n, gk), only_k)
    gn[4] = 0.0                                                                      # one row's cotangents all zero: that row alone is off
    gk[4] = 0.0
    rec = host_records(lib, P, fwd, gn, gk)
    assert on[4] and rec[4, 12] == 0.0 and not rec[4, :9].any() and np.array_equal(rec[:, 12] != 0, on & (np.arange(65) != 4))
    assert ir.same_bits(rec[:, 9:12], P.astype(np.float64))


# ------------------------------------------------------------------ the records against torch autograd
def autograd(P, radius, rows, viewpoint, min_neighbors, gn, gk):
    """the float64 composition's gradient of sum(gn . n) + sum(gk curvature) -> (grad (m, 3), dL/dC symmetrised (m, 3, 3))"""
    x = torch.from_numpy(np.where(np.isfinite(P[:, :3]), P[:, :3], 0.0).astype(np.float64)).requires_grad_(True)
    out = nbr.composition(x, radius, rows, viewpoint, min_neighbors, points=P)
    out["C"].retain_grad()
    loss = (out["normals"] * torch.from_numpy(gn.astype(np.float64))).sum() + (out["curv"] * torch.from_numpy(gk.astype(np.float64))).sum()
    loss.backward()
    G = out["C"].grad.numpy()
    return x.grad.numpy(), 0.5 * (G + G.transpose(0, 2, 1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["cube 300", "cube 65 rows", "sheet", "clusters"])
def test_records_against_autograd(lib, dtype, case):
    if case == "cube 300":
        P, rows, r, vp, min_nb = ibc.cube(21, 300, dtype), None, None, None, 3
        r = ibc.ball_radius(P, 14)
    elif case == "cube 65 rows":
        P, rows, vp, min_nb = ibc.cube(22, 65, dtype), 50, [0.5, 0.5, 3.0], 5
        P[3, 1], P[9, 0], P[11] = np.nan, np.inf, P[10]
        r = ibc.ball_radius(P[:50], 9)
    elif case == "sheet":
        P, rows, r, vp, min_nb = nbc.sheet().astype(dtype), None, nbc.SHEET_RADIUS, None, 3
    else:
        P, rows, r, vp, min_nb = nbc.clusters(41, dtype), None, nbc.CLUSTER_RADIUS, [0.0, 0.0, 50.0], 3
    m = P.shape[0]
    gn, gk = cotangents(5, m, dtype)
    fwd = host_forward(lib, P, r, rows, vp, min_nb)
    rec = host_records(lib, P, fwd, gn, gk)
    grad, _ = host_gather(lib, P, r, rec, rows)
    ref = nbr.forward_ref(P, r, rows, vp, min_nb)
    lam = ref["lam"]
    on = (ref["count"] >= min_nb) & (lam.sum(1) > 0)
    gap = (lam[on, 1] - lam[on, 0]) / lam[on].sum(1)
    print("%s %s: rows on %d of %d, smallest relative gap %.3g" % (case, np.dtype(dtype).name, on.sum(), m, gap.min()))
    assert on.sum() > m // 2 and gap.min() > 1e-3                                   # (every row on is far from the tau cut)
    assert rec[on, 12].all() and not rec[~on, 12].any()
    want_grad, want_G = autograd(P, r, rows, vp, min_nb, gn, gk)
    G = rec[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(m, 3, 3)
    assert np.allclose(G[on], want_G[on], rtol=RTOL, atol=ATOL)
    assert np.allclose(grad.astype(np.float64), want_grad, rtol=RTOL, atol=ATOL)
    assert np.abs(want_grad).max() > 1e-2 and not grad[ref["count"] == 0].any()


# ------------------------------------------------------------------ the conditions of the GPU tests' designed cases, on the references alone
def test_sheet_conditions():
    cond = nbc.sheet_conditions()
    print("sheet: counts %d .. %d, smallest relative gap %.3g, nearest pair to the border %.3g" % cond)
    assert cond[0] >= 3 and cond[1] <= 16 and cond[2] >= 0.02 and cond[3] >= 1.5e-3


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", nbc.CLUSTER_SEEDS)
def test_cluster_conditions(dtype, seed):
    """every ball holds exactly its cluster, the eigenvalues are separated and no pair is near the border: the whole-ball form and
    estimate_normals(k=12) see the same member sets"""
    own, count_min, count_max, gap, border = nbc.cluster_conditions(seed, dtype)
    print("clusters seed %d %s: counts %d .. %d, smallest relative gap %.3g, nearest pair to the border %.3g"
          % (seed, np.dtype(dtype).name, count_min, count_max, gap, border))
    assert own and count_min == count_max == 12 and gap >= 0.1 and border >= 0.7
