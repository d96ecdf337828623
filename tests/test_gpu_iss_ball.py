"""iss_saliency_ball / iss_keypoints_ball / compute_iss_keypoints(whole_ball=True) on the MI355X (dicp_amd/iss.py; csrc/iss_ball.hip)
against the numpy restatement tests/iss_ball_ref.py: eigenvalues, saliency and counts bit for bit, the keypoint mask exactly, float32 and
float64.

1  tile and wave edges: m in {1, 2, 63, 64, 65, 300}, two clouds of different row counts per call, dead rows and extra columns holding
   NaN, c in {3, 6}, balls of about 4, 40 and 150 rows, the non-max radius smaller and larger than the salient one;
2  the designed clouds of tests/iss_cases.py as whole-ball cases, a cloud with no rows, and the layouts of the coverage claim
   (tests/iss_ball_cases.py: rows exactly at distance R, a radius that rounds down in float32, enlarged edges, a flat grid);
3  single clouds, lists and CPU tensors against the batch, no gradient, a call in a captured graph;
4  compute_iss_keypoints(whole_ball=True) against its steps, its index, its gradient;
5  the cross-check with the k-slot form where every ball fits 32 slots;  6  the cube-corner scene at a radius whose balls do not.

Where a grid's plan enlarged an edge or went flat, the reference takes the edges from the library's own plan (read back from the CellGrid
the front end builds); tests/iss_ball_ref.py asserts that the simple rule is used wherever the plan did not.
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import iss as iss_module
from dicp_amd.ball import ball_query
from dicp_amd.filter import select_rows
from dicp_amd.iss import compute_iss_keypoints, iss_keypoints, iss_keypoints_ball, iss_saliency, iss_saliency_ball

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iss_ball_cases as ibc  # noqa: E402
import iss_ball_ref as ibr  # noqa: E402
import iss_cases as ic  # noqa: E402
import iss_ref as ir  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def device_plans(Pd, rows_t, radius):
    """the plans of the grid the front end builds for this batch and radius -> [(edges (3,), enlarged, flat)] per cloud (csrc/dicp_ball.h:
    BallPlan -- o[3], s[3], R, r2 of T, then hi[3] int64, wy, wz, cnt, flat int32)"""
    grid = iss_module._ball_grid(Pd, rows_t, radius)
    raw = host(grid.plans)
    dt = host(Pd).dtype
    ts = dt.itemsize
    out = []
    for b in range(raw.shape[0]):
        f = raw[b, :8 * ts].copy().view(dt)
        ints = raw[b, 8 * ts + 24:8 * ts + 40].copy().view(np.int32)
        edges, R, flat = f[3:6], f[6], bool(ints[3])
        out.append((edges, flat or bool((edges != R).any()), flat))
    return out


def reference(P, rows, rows_t, r1, r2, **params):
    Pd = dev(P)
    plans = device_plans(Pd, rows_t, max(r1, r1 if r2 is None else r2))
    return ibr.keypoints_ball_ref_batch(P, r1, r2, rows, plans=[p if (p[1] or p[2]) else None for p in plans], **params)


def check(P, rows, r1, r2=None, **params):
    """both front ends on one batch against the reference -> the reference of iss_keypoints_ball.  iss_saliency_ball builds its grid at
    ITS radius, iss_keypoints_ball at the larger of the two: where the non-max radius is the larger, the member order -- and with it the
    last bits of the sums -- is that of another grid, and each front end is held to the reference in its own order."""
    rows_t = None if rows is None else torch.tensor(np.asarray(rows), dtype=torch.int32).cuda()
    Pd = dev(P)
    ref = reference(P, rows, rows_t, r1, r2, **params)
    alone = ref if (r2 is None or r2 <= r1) else reference(P, rows, rows_t, r1, None, **params)
    sal, eig, cnt = iss_saliency_ball(Pd, r1, rows=rows_t, return_eigenvalues=True, return_counts=True, **params)
    assert sal.shape == P.shape[:2] and eig.shape == P.shape[:2] + (3,) and cnt.shape == sal.shape and cnt.dtype == torch.int32
    assert sal.dtype == Pd.dtype and eig.dtype == Pd.dtype and not sal.requires_grad and not eig.requires_grad
    mask, sal2 = iss_keypoints_ball(Pd, r1, r2, rows=rows_t, return_saliency=True, **params)
    assert mask.dtype == torch.bool and mask.shape == sal.shape and not mask.requires_grad
    got = dict(eig=host(eig), sal=host(sal), count=host(cnt))
    for key in ("count", "eig", "sal"):
        assert ir.same_bits(got[key], alone[key]), key
    assert ir.same_bits(host(mask), ref["mask"]) and ir.same_bits(host(sal2), ref["sal"])
    assert np.array_equal(ref["count"], alone["count"])
    return ref


def padded(clouds, cols):
    """clouds [(points (m_b, 3), rows_b)] -> P (N, m, cols) with NaN in dead rows, pad rows and extra columns, rows (N,)"""
    m = max(c[0].shape[0] for c in clouds)
    P = np.full((len(clouds), m, cols), np.nan, dtype=clouds[0][0].dtype)
    for b, (pts, r) in enumerate(clouds):
        P[b, :r, :3] = pts[:r, :3]
    return P, np.array([c[1] for c in clouds], dtype=np.int32)


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 300])
def test_tile_edges(dtype, m):
    for q, members in enumerate((4, 40, 150)):
        a, b = ibc.cube(100 * m + q, m, dtype), ibc.cube(100 * m + q + 50, m, dtype)
        if m >= 63:
            a[3, 1], a[9, 0], a[11] = np.nan, np.inf, a[10]                        # dead rows inside the cloud, an exact duplicate
        P, rows = padded([(a, m), (b, m - m // 3)], 3 if q % 2 == 0 else 6)
        r1 = ibc.ball_radius(a, members) if m > 2 else 0.8
        for r2 in (0.7 * r1, 1.3 * r1):
            ref = check(P, rows, r1, r2)
        live = ref["count"][0] > 0
        if m == 300:
            assert abs(np.median(ref["count"][0][live]) - 1 - members) <= 0.5 * members      # (the ball holds what the case says)
            assert (members <= 31) == (ref["count"].max() <= 32)                             # 40 and 150: beyond the k-slot form
            assert ref["mask"].sum() >= 1 and (ref["sal64"] > 0).sum() > ref["mask"].sum()
        if m >= 63:
            assert not ref["count"][0, 3] and not ref["count"][0, 9] and not ref["count"][1, m - m // 3:].any()


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["duplicates", "planar", "collinear", "counts", "ratio", "only_itself", "non_finite"])
def test_designed_clouds(dtype, name):
    pts, rows, r, params = ibc.designed(dtype)[name]
    P, rw = padded([(pts, rows), (ibc.cube(9, 12, dtype), 0)], 3)                  # with a cloud that has no rows
    ref = check(P, rw, r, **params)
    sal, cnt, mask, eig = ref["sal64"][0], ref["count"][0], ref["mask"][0], ref["eig"][0].astype(np.float64)
    assert not ref["count"][1].any() and not ref["eig"][1].any() and not ref["mask"][1].any()
    if name == "duplicates":
        assert sal[0] > 0 and sal[0] == sal[1] and cnt[0] == cnt[1] == 10 and not mask[1]
    if name == "planar":
        assert (eig[:8, 0] == 0.0).all() and (eig[:8, 1] > 0).all() and not sal.any() and not mask.any()
    if name == "collinear":
        assert not eig[:, :2].any() and (eig[:8, 2] > 0).all() and not sal.any()
    if name == "counts":
        assert list(cnt[:9]) == [5] * 5 + [4] * 4 and sal[0] > 0 and not sal[5:].any()
        four = check(P, rw, r, min_neighbors=4)
        assert four["sal64"][0, 5] > 0
    if name == "ratio":
        assert eig[0, 1] == 0.25 * eig[0, 2] and eig[0, 0] == 0.25 * eig[0, 1] and sal[0] > 0
        for g21, g32, salient in ((0.25, 0.5, False), (0.5, 0.25, False), (0.5, 0.5, True)):
            assert bool(check(P, rw, r, gamma21=g21, gamma32=g32)["sal64"][0, 0] > 0) == salient
    if name == "only_itself":
        assert list(cnt[:6]) == [1, 1, 0, 0, 0, 0] and not eig.any() and not mask.any()
    if name == "non_finite":
        assert list(cnt[:11]) == [9] * 9 + [0, 0] and sal[0] > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ibc.LAYOUT_NAMES)
def test_layouts(dtype, name):
    pts, r1, r2 = ibc.layouts(dtype)[name]
    plans = device_plans(dev(pts[None]), None, max(r1, r2))
    assert (plans[0][1], plans[0][2]) == (name in ("two clusters", "far outlier", "flat"), name == "flat")
    ref = check(pts[None], None, r1, r2)
    brute = ibr.members_brute(pts, None, r1)
    assert np.array_equal(ref["count"][0], 1 + brute.sum(axis=1))                  # (the reference's members are the brute force's)


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("dtype", DTYPES)
def test_forms(dtype):
    rows = [90, 61, 75]
    P, rw = padded([(ibc.cube(51 + b, 90, dtype), r) for b, r in enumerate(rows)], 4)
    r1, r2 = 0.5, 0.4
    ref = check(P, rw, r1, r2)
    assert ref["mask"].sum() >= 3 and ref["count"].max() > 12
    for b, r in enumerate(rows):
        mask, sal = iss_keypoints_ball(dev(P[b, :r]), r1, r2, return_saliency=True)
        assert mask.shape == (r,) and np.array_equal(host(mask), ref["mask"][b, :r]) and ir.same_bits(host(sal), ref["sal"][b, :r])
        eig = iss_saliency_ball(dev(P[b, :r]), r1, return_eigenvalues=True)[1]
        assert eig.shape == (r, 3) and ir.same_bits(host(eig), ref["eig"][b, :r])
    masks, sals = iss_keypoints_ball([dev(P[b, :r]) for b, r in enumerate(rows)], r1, r2, return_saliency=True)
    assert isinstance(masks, list) and all(np.array_equal(host(o), ref["mask"][b, :r]) for b, (o, r) in enumerate(zip(masks, rows)))
    assert all(ir.same_bits(host(o), ref["sal"][b, :r]) for b, (o, r) in enumerate(zip(sals, rows)))
    mask_c, sal_c = iss_keypoints_ball(torch.from_numpy(P), r1, r2, rows=torch.tensor(rows), return_saliency=True)
    assert not mask_c.is_cuda and not sal_c.is_cuda and np.array_equal(mask_c.numpy(), ref["mask"]) and ir.same_bits(sal_c.numpy(), ref["sal"])
    cnt_c = iss_saliency_ball(torch.from_numpy(P), r1, rows=torch.tensor(rows), return_counts=True)[1]
    assert not cnt_c.is_cuda and np.array_equal(cnt_c.numpy(), ref["count"])
    x = dev(P[0, :90]).requires_grad_(True)
    mask, sal = iss_keypoints_ball(x, r1, r2, return_saliency=True)
    assert not mask.requires_grad and not sal.requires_grad and ir.same_bits(host(sal), ref["sal"][0])
    assert not iss_saliency_ball(x, r1).requires_grad


def test_captured_call():
    rows = [400, 333]

    def data(seed):
        P, rw = padded([(ibc.cube(seed + b, 400, np.float32), r) for b, r in enumerate(rows)], 3)
        return {"P": dev(P), "rows": torch.tensor(rw, dtype=torch.int32).cuda()}

    def run(s):
        sal, eig, cnt = iss_saliency_ball(s["P"], 0.4, rows=s["rows"], return_eigenvalues=True, return_counts=True)
        mask = iss_keypoints_ball(s["P"], 0.4, 0.3, rows=s["rows"])
        return sal, eig, cnt, mask
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
    for seed in (20, 30):
        fresh = data(seed)
        for key, t in fresh.items():
            static[key].copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(fresh)
        torch.cuda.synchronize()
        assert all(ir.same_bits(host(c), host(e)) for c, e in zip(captured, eager))
        assert captured[3].sum() > 0 and int(captured[2].max()) > 32


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("dtype", DTYPES)
def test_compute_iss_keypoints_whole_ball(dtype):
    rows = [400, 333]
    P, rw = padded([(ibc.cube(61 + b, 400, dtype), r) for b, r in enumerate(rows)], 4)
    P[..., 3] = np.arange(P.shape[0] * P.shape[1]).reshape(P.shape[:2])            # a column carried along
    Pd, rt = dev(P), torch.tensor(rw).cuda()
    r1, r2 = 0.45, 0.3
    mask = iss_keypoints_ball(Pd, r1, r2, rows=rt)
    want, want_rows, want_index = select_rows(Pd, mask, rows=rt, return_index=True)
    ref = ibr.keypoints_ball_ref_batch(P, r1, r2, rw)
    assert np.array_equal(host(mask), ref["mask"]) and ref["mask"].sum(axis=1).min() >= 3 and ref["count"].max() > 32
    got, got_rows, index = compute_iss_keypoints(Pd, r1, r2, rows=rt, return_index=True, whole_ball=True)
    assert torch.equal(got, want) and torch.equal(got_rows, want_rows) and torch.equal(index, want_index)
    assert got.shape == Pd.shape and got_rows.dtype == torch.int32 and list(host(got_rows)) == list(ref["mask"].sum(axis=1))
    for b in range(2):
        n = int(got_rows[b])
        assert list(host(index[b, :n])) == list(np.flatnonzero(ref["mask"][b])) and bool((index[b, n:] == -1).all())
        assert ir.same_bits(host(got[b, :n]), P[b][ref["mask"][b]]) and not host(got[b, n:]).any()
    same_k = compute_iss_keypoints(Pd, r1, r2, k=3, rows=rt, whole_ball=True)       # k is ignored
    assert len(same_k) == 2 and torch.equal(same_k[0], got)
    two = compute_iss_keypoints(Pd, r1, rows=rt, whole_ball=True)                   # non_max_radius=None: the salient radius
    assert torch.equal(two[0], compute_iss_keypoints(Pd, r1, r1, rows=rt, whole_ball=True)[0])
    assert not torch.equal(compute_iss_keypoints(Pd, r1, r2, rows=rt)[0], got)      # whole_ball=False: the k-slot path, other keypoints here
    x = Pd.clone().requires_grad_(True)
    out, _ = compute_iss_keypoints(x, r1, r2, rows=rt, whole_ball=True)
    assert out.requires_grad
    w = torch.arange(1, out.numel() + 1, dtype=out.dtype, device=out.device).reshape(out.shape)
    (out * w).sum().backward()
    g = host(x.grad)
    assert (g[ref["mask"]] != 0).all() and not g[~ref["mask"]].any()


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", [31, 32])
def test_cross_check_with_the_k_slot_form(dtype, seed):
    """On tests/iss_ball_cases.py's cross_scene every ball holds at most 31 other rows, so ball_query(k=32) -> iss_saliency sees the SAME
    members as iss_saliency_ball: the counts must be equal exactly.  The two forms differ only in the order of their sums.

    The bound on the eigenvalues (ibc.eigenvalue_bound), derived -- not fitted.  u = 2^-53, n <= 32 members inside the radius r, so every
    |q_a| <= rho with rho^2 <= 1.01 r^2; gamma_j = j u / (1 - j u).
      mean: a recursive sum of n - 1 terms in either order errs by at most gamma_(n-1) sum|q_a|, the division adds one rounding: each
        form's mu is within gamma_n rho of the exact mean, the two within 2 gamma_n rho of each other.
      six sums: with d = q - mu (|d_a| <= 2 rho), each form's entry errs by at most gamma_(n+3) mean|d_a d_b| <= 4 gamma_(n+3) rho^2
        against the exact entry for ITS mu (the subtraction, the product, n additions, the division); and moving mu by delta moves an
        exact entry by at most 2 * 2 rho * delta + delta^2 <= 8.1 gamma_n rho^2.  Two forms: 2 * 4 + 8.1 <= 16 gamma_(n+3) rho^2 an entry.
      Weyl: the eigenvalues of two symmetric 3 x 3 matrices differ by at most the 2-norm of their difference, at most 3 times the
        largest entry: 48 gamma_(n+3) rho^2.
      Jacobi: each form's computed eigenvalues are within 27.5 u trace of its matrix's (the accuracy tests/test_iss_host.py asserts): twice.
      float32 outputs: each rounded once, 2^-24 of an eigenvalue <= trace, twice.
    Total 48 gamma_(n+3) 1.01 r^2 + 55 u trace (+ 2^-23 trace in float32).

    The masks are compared only on rows whose threshold tests and saliency comparisons have more than twice that margin in the float64
    reference (ibc.excluded_rows); tests/test_iss_ball_host.py asserts on the CPU that those rows are at most 2 % of a case."""
    P, r = ibc.cross_scene(seed, dtype)
    m = P.shape[0]
    Pd = dev(P[None])
    _, idx, counts = ball_query(Pd, Pd, r, k=ibc.K, return_counts=True)
    assert int(counts.max()) <= ibc.K
    sal_k, eig_k, cnt_k = iss_saliency(Pd, idx, radius=r, return_eigenvalues=True, return_counts=True)
    mask_k = iss_keypoints(Pd, idx, salient_radius=r, non_max_radius=r)
    sal_b, eig_b, cnt_b = iss_saliency_ball(Pd, r, return_eigenvalues=True, return_counts=True)
    mask_b = iss_keypoints_ball(Pd, r)
    assert torch.equal(cnt_k, cnt_b) and int(cnt_b.max()) > 16
    ref = ibr.keypoints_ball_ref(P, r)
    trace = ref["eig"].astype(np.float64).sum(axis=1).max()
    bound = ibc.eigenvalue_bound(r, int(ref["count"].max()), trace, dtype)
    diff = np.abs(host(eig_k).astype(np.float64) - host(eig_b).astype(np.float64)).max()
    print("seed %d %s: |eigenvalue difference| max %.3g, bound %.3g" % (seed, np.dtype(dtype).name, diff, bound))
    assert diff <= bound
    out = ibc.excluded_rows(P, ref, r, bound, ibr.full_index(ref["order"], m))
    assert out.sum() <= 0.02 * m
    assert np.array_equal(host(mask_k)[0][~out], host(mask_b)[0][~out]) and int(mask_b.sum()) >= 2


# ------------------------------------------------------------------ 6
CORNER_SEEDS = (1, 2, 3)
CORNER_BALL_RADIUS = 1.0


def test_corner_scene_whole_ball():
    """The cube-corner scene of tests/iss_cases.py at radius 1.0: a ball on a face holds about 50 rows, near an edge more -- beyond the
    32 slots of the k-slot form, which then sees a truncated, nearer neighbourhood.  The whole-ball keypoints equal the reference's; rows
    farther than the radius from all three edges have saliency exactly 0 (one plane); and the keypoints differ from the k = 32 form's."""
    scenes = [ic.corner_scene(seed) for seed in CORNER_SEEDS]
    P = np.stack([s[0] for s in scenes])
    Pd = dev(P)
    r = CORNER_BALL_RADIUS
    ref = check(P, None, r)
    assert np.median(ref["count"]) > 33
    kp, rows_out, index = compute_iss_keypoints(Pd, r, return_index=True, whole_ball=True)
    kp32, rows32, index32 = compute_iss_keypoints(Pd, r, k=32, return_index=True)
    for b, (pts, edge) in enumerate(scenes):
        n = int(rows_out[b])
        rows = host(index[b, :n])
        assert list(rows) == list(np.flatnonzero(ref["mask"][b])) and n >= 1
        assert not ref["sal64"][b][edge > r].any() and (edge[rows] <= r).all()
        print("seed %d: %d whole-ball keypoints, %d with k = 32" % (CORNER_SEEDS[b], n, int(rows32[b])))
    assert not torch.equal(index, index32)
