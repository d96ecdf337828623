"""CPU checks of the whole-ball ISS keypoints (dicp_amd/iss.py: iss_saliency_ball / iss_keypoints_ball) that need no GPU.

``dicp_amd/csrc/dicp_iss_ball.h`` -- the member walk and the two passes the HIP kernels execute -- is compiled with g++ through
tests/hostcheck/iss_ball_check.cpp, run on a host-sorted grid and held to tests/iss_ball_ref.py: counts, eigenvalues and saliency bit for
bit, the mask exactly.  The COVERAGE CLAIM of the header is held separately: the rows the walk visits and iss_member accepts are compared
with an O(m^2) brute force of the double rule, on the layouts where a cell range could lose a member (points exactly at distance R, a
float32 radius that rounds down, ranges of four cells, a wall, clusters whose keys need enlarged edges, a far outlier, a flat grid).
The comparison is shown to refuse members taken in row order.  The cap of the GPU cross-check with the k-slot form (rows left out of the
mask comparison: at most 2 % of a case) is asserted here on the two numpy references alone.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostbuild  # noqa: E402
import iss_ball_cases as ibc  # noqa: E402
import iss_ball_ref as ibr  # noqa: E402
import iss_ref as ir  # noqa: E402

RIGHT, ROW_ORDER = 0, 1
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def lib():
    so = hostbuild.build("iss_ball_check.cpp", "iss_ball_check")
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    so.ibc_cloud.argtypes, so.ibc_cloud.restype = [i32, vp, i32, i32, i32, f64, f64, f64, f64, i32, i32, vp, vp, vp, vp, vp, vp], None
    so.ibc_members.argtypes, so.ibc_members.restype = [i32, vp, i32, i32, i32, f64, f64, vp, vp], None
    so.ibc_plan.argtypes, so.ibc_plan.restype = [i32, vp, i32, i32, i32, f64, vp, vp], None
    so.ibc_radii.argtypes, so.ibc_radii.restype = [i32, f64, vp], None
    return so


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_plan(lib, pts, rows, radius):
    """the host build's plan of one cloud at the grid radius of `radius` -> (edges (3,) of the points' dtype, enlarged, flat)"""
    pts = np.ascontiguousarray(pts)
    edges, flags = np.zeros(3), np.zeros(3, np.int32)
    lib.ibc_plan(int(pts.dtype == np.float64), _p(pts), pts.shape[1], pts.shape[0], pts.shape[0] if rows is None else rows, float(radius),
                 _p(edges), _p(flags))
    return edges.astype(pts.dtype), bool(flags[0]), bool(flags[1])


def host(lib, pts, r1, r2=None, rows=None, gamma21=0.975, gamma32=0.975, min_neighbors=5, variant=RIGHT):
    """the header's two passes on one cloud -> dict eig, sal, count, mask, order (the sorted rows), stats"""
    pts = np.ascontiguousarray(pts)
    m = pts.shape[0]
    eig, sal = np.zeros((m, 3), pts.dtype), np.zeros(m, pts.dtype)
    cnt, mask, order, stats = np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros(m, np.int64), np.zeros(5, np.int64)
    lib.ibc_cloud(int(pts.dtype == np.float64), _p(pts), pts.shape[1], m, m if rows is None else rows, float(r1), float(r1 if r2 is None else r2),
                  gamma21, gamma32, min_neighbors, variant, _p(eig), _p(sal), _p(cnt), _p(mask), _p(order), _p(stats))
    return dict(eig=eig, sal=sal, count=cnt, mask=mask.astype(bool), order=order[order >= 0], stats=stats)


def host_members(lib, pts, rows, grid_radius, radius):
    pts = np.ascontiguousarray(pts)
    m = pts.shape[0]
    mem, stats = np.zeros((m, m), np.uint8), np.zeros(6, np.int64)
    lib.ibc_members(int(pts.dtype == np.float64), _p(pts), pts.shape[1], m, m if rows is None else rows, float(grid_radius), float(radius), _p(mem),
                    _p(stats))
    return mem.astype(bool), stats


def ref(lib, pts, r1, r2=None, rows=None, **kw):
    """the numpy restatement, with the plan of the host build where the layout needs one"""
    plan = host_plan(lib, pts, rows, max(r1, r1 if r2 is None else r2))
    return ibr.keypoints_ball_ref(pts, r1, r2, rows, plan=plan if (plan[1] or plan[2]) else None, **kw), plan


# ------------------------------------------------------------------ the radii
@pytest.mark.parametrize("r", [0.06, 0.1, 0.7, 1.0, 1e-30, 1e-46, 3.3e38, 1e39, 1e150])
def test_grid_radius_and_half_width(lib, r):
    out = np.zeros(2)
    for f64, dtype in ((0, np.float32), (1, np.float64)):
        lib.ibc_radii(f64, r, _p(out))
        rt = ibr.grid_radius(r, dtype)
        assert out[0] == float(rt) and np.isfinite(out[0])
        assert out[0] >= r or (dtype == np.float32 and r > float(np.finfo(np.float32).max) and out[0] == float(np.finfo(np.float32).max))
        assert out[1] == float(ibr.ball_R(rt)) and (out[1] > r or not np.isfinite(out[1]))
    assert float(np.float32(0.06)) < 0.06 < float(ibr.grid_radius(0.06, np.float32))               # (a conversion that rounds down)


# ------------------------------------------------------------------ the header against the reference
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,rows,members,cols", [(300, None, 4, 3), (300, 211, 40, 4), (65, None, 12, 3), (300, None, 150, 6), (40, 33, 8, 3),
                                                 (2, None, 1, 3), (1, None, 1, 3)])
def test_random_clouds(lib, dtype, m, rows, members, cols):
    P = np.full((m, cols), np.nan, dtype=dtype)
    P[:, :3] = ibc.cube(m + members, m, dtype)
    if m >= 40:
        P[3, 1], P[9, 0], P[11] = np.nan, np.inf, P[10]
    r1 = ibc.ball_radius(P[:rows], members) if m > 2 else 0.5
    for r2 in (None, 0.7 * r1, 1.3 * r1):
        want, plan = ref(lib, P, r1, r2, rows)
        got = host(lib, P, r1, r2, rows)
        assert not plan[1] and not plan[2]
        assert ir.same_bits(got["order"], want["order"])
        assert ir.same(got, want)
    live = want["count"] > 0
    if m >= 65:
        assert abs(np.median(want["count"][live]) - 1 - members) <= max(2, 0.5 * members)          # (the ball holds what the case says)
        assert not want["count"][3] and not want["count"][9] and want["count"][10] == want["count"][11]
    if m == 300 and 8 <= members <= 40:
        assert (want["sal64"] > 0).sum() > 10 and 1 <= want["mask"].sum() < (want["sal64"] > 0).sum()
    if rows is not None:
        assert not want["count"][rows:].any() and not want["mask"][rows:].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["duplicates", "planar", "collinear", "counts", "ratio", "only_itself", "non_finite"])
def test_designed_clouds(lib, dtype, name):
    P, rows, r, params = ibc.designed(dtype)[name]
    want, _ = ref(lib, P, r, None, rows, **params)
    assert ir.same(host(lib, P, r, None, rows, **params), want)
    sal, cnt, mask, eig = want["sal64"], want["count"], want["mask"], want["eig"].astype(np.float64)
    if name == "duplicates":
        assert sal[0] > 0 and sal[0] == sal[1] and cnt[0] == cnt[1] == 10 and not mask[1]           # an exact tie: the lower row alone can stay
        assert bool(mask[0]) == bool(sal[0] >= sal.max())
    if name == "planar":
        assert (eig[:, 0] == 0.0).all() and (eig[:, 1] > 0).all() and not sal.any() and not mask.any() and (cnt == 8).all()
    if name == "collinear":
        assert not eig[:, :2].any() and (eig[:, 2] > 0).all() and not sal.any()
    if name == "counts":
        assert list(cnt) == [5] * 5 + [4] * 4 and sal[0] > 0 and not sal[5:].any()
        four, _ = ref(lib, P, r, None, rows, min_neighbors=4)
        assert four["sal64"][5] > 0 and ir.same(host(lib, P, r, None, rows, min_neighbors=4), four)      # one below: the count alone decided
    if name == "ratio":
        assert eig[0, 1] == 0.25 * eig[0, 2] and eig[0, 0] == 0.25 * eig[0, 1] and sal[0] > 0
        for g21, g32, salient in ((0.25, 0.5, False), (0.5, 0.25, False), (0.5, 0.5, True)):
            at, _ = ref(lib, P, r, None, rows, gamma21=g21, gamma32=g32)
            assert bool(at["sal64"][0] > 0) == salient and ir.same(host(lib, P, r, None, rows, gamma21=g21, gamma32=g32), at)
    if name == "only_itself":
        assert list(cnt) == [1, 1, 0, 0, 0, 0] and not eig.any() and not mask.any()
    if name == "non_finite":
        assert list(cnt) == [9] * 9 + [0, 0] and sal[0] > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_cloud_with_no_live_rows(lib, dtype):
    P = ibc.cube(1, 12, dtype)
    got = host(lib, P, 0.5, None, rows=0)
    assert not got["count"].any() and not got["eig"].any() and not got["mask"].any() and got["order"].size == 0
    assert ir.same(got, ibr.keypoints_ball_ref(P, 0.5, None, 0))


# ------------------------------------------------------------------ the coverage claim
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ibc.LAYOUT_NAMES)
def test_layouts(lib, dtype, name):
    """membership against the O(m^2) brute force of the double rule for both passes' radii on the grid of the larger one, then every
    output against the restatement in the host plan's order"""
    P, r1, r2 = ibc.layouts(dtype)[name]
    big = max(r1, r2)
    for r in (r1, r2):
        mem, stats = host_members(lib, P, None, big, r)
        brute = ibr.members_brute(P, None, r)
        assert np.array_equal(mem, brute), name
        assert stats[4] == 0 and brute.sum() > 0                                # no row visited twice; the case has members
        print("%-20s %s r=%-8g visited/row %7.1f members/row %6.1f span %d enlarged %d flat %d other-cell members %d"
              % (name, np.dtype(dtype).name, r, stats[0] / P.shape[0], brute.sum() / P.shape[0], stats[1], stats[2], stats[3], stats[5]))
        if name.startswith("lattice r="):
            d2 = ((P[171].astype(np.float64) - P.astype(np.float64)) ** 2).sum(-1)
            at = d2 == np.float64(r) * np.float64(r)
            if r in (1.0, 2.0):
                assert at.sum() == 6 and mem[171][at].all()                     # rows EXACTLY at distance R are members
            assert stats[5] > 0
        if name in ("two clusters", "far outlier"):
            assert stats[2] == 1 and stats[3] == 0
        if name == "flat":
            assert stats[3] == 1 and stats[0] == (P.shape[0]) ** 2
    if name == "radius rounds down":
        assert float(P.dtype.type(r1)) < r1 or P.dtype == np.float64
        near = ibr.members_brute(P, None, r1)[:6, 300:].sum()
        assert near >= 3                                                        # the rows float32(r) away ARE members under the double rule
    want, plan = ref(lib, P, r1, r2)
    got = host(lib, P, r1, r2)
    assert (plan[1] or plan[2]) == (name in ("two clusters", "far outlier", "flat"))
    assert ir.same_bits(got["order"], want["order"])
    assert ir.same(got, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_range_of_four_cells_per_axis(lib, dtype):
    """a pass whose radius is 1.5 times the grid's: the claim holds for any cell edge, the range spans four cells and more"""
    P = ibc.cube(21, 400, dtype, scale=(0.5, 0.5, 0.5))
    mem, stats = host_members(lib, P, None, 0.1, 0.15)
    assert stats[1] >= 4 and np.array_equal(mem, ibr.members_brute(P, None, 0.15)) and stats[4] == 0
    if dtype == np.float32:                                 # 2.5 km out, p +- R in float32 rounds by 1.2e-4: four cells at the grid's OWN radius
        Q = ibc.layouts(dtype)["cube at 2500"][0]
        mem, stats = host_members(lib, Q, None, 0.08, 0.08)
        brute = ibr.members_brute(Q, None, 0.08)
        assert stats[1] >= 4 and brute.sum() > 100 and np.array_equal(mem, brute) and stats[4] == 0


# ------------------------------------------------------------------ the comparison refuses a wrong order
def test_refuses_members_in_row_order(lib):
    """(float64: rounded to float32 the two orders give the same outputs on every row of such a cloud)"""
    dtype = np.float64
    P = ibc.cube(5, 300, dtype)
    r = ibc.ball_radius(P, 40)
    right, wrong = ibr.keypoints_ball_ref(P, r), ibr.keypoints_ball_ref(P, r, row_order=True)
    got = host(lib, P, r, variant=ROW_ORDER)
    assert ir.same(host(lib, P, r), right)
    assert ir.same_bits(wrong["count"], right["count"]) and not ir.same_bits(wrong["eig"], right["eig"])
    assert ir.same(got, wrong, keys=("eig", "sal", "count")) and not ir.same(got, right)
    assert np.allclose(wrong["eig"], right["eig"], rtol=1e-5, atol=0)           # (the same members: only the order of the sums differs)


# ------------------------------------------------------------------ the cap of the GPU cross-check, on the two references alone
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", [31, 32])
def test_cross_check_cap(dtype, seed):
    """test_gpu_iss_ball.py compares the masks of the k-slot form and of the whole-ball form only on rows with more margin than the
    derived eigenvalue bound; the rows left out may be at most 2 % of a case.  Here: the two numpy references agree within that bound,
    have equal counts, and the excluded rows stay under the cap."""
    P, r = ibc.cross_scene(seed, dtype)
    m = P.shape[0]
    _, knn = ir.knn_self(P, ibc.K)
    slot = ir.keypoints_ref(P, knn, None, r, r)
    ball = ibr.keypoints_ball_ref(P, r)
    assert ir.same_bits(slot["count"], ball["count"]) and ball["count"].max() <= ibc.K and np.median(ball["count"]) >= 8 and ball["count"].max() > 16
    trace = ball["eig"].astype(np.float64).sum(axis=1).max()
    bound = ibc.eigenvalue_bound(r, int(ball["count"].max()), trace, dtype)
    diff = np.abs(slot["eig"].astype(np.float64) - ball["eig"].astype(np.float64)).max()
    print("seed %d %s: |eig difference| max %.3g, bound %.3g" % (seed, np.dtype(dtype).name, diff, bound))
    assert diff <= bound
    out = ibc.excluded_rows(P, ball, r, bound, ibr.full_index(ball["order"], m))
    print("rows excluded: %d of %d" % (out.sum(), m))
    assert out.sum() <= 0.02 * m
    assert np.array_equal(slot["mask"][~out], ball["mask"][~out]) and ball["mask"].sum() >= 2
