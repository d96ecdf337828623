"""CPU checks of the whole-ball FPFH descriptor (dicp_amd/fpfh.py: fpfh_features_ball / compute_fpfh(whole_ball=True)) that need no GPU.

``dicp_amd/csrc/dicp_fpfh_ball.h`` -- the near list and the two passes the HIP kernels execute -- is compiled with g++ through
tests/hostcheck/fpfh_ball_check.cpp, run serially on a host-sorted grid and held to tests/fpfh_ball_ref.py: the pair counts integer for
integer, the descriptor bit for bit, float32 and float64.  The reference itself is anchored to tests/fpfh_ref.py wherever no count passes
255.  The comparison is shown to refuse a near list taken in row order, and the bound of the GPU cross-check with the k-slot form is
asserted here on the two numpy references alone.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_ball_cases as fbc  # noqa: E402
import fpfh_ball_ref as fbr  # noqa: E402
import fpfh_cases as fc  # noqa: E402
import fpfh_ref as fr  # noqa: E402
import hostbuild  # noqa: E402
import iss_ball_cases as ibc  # noqa: E402
import iss_ball_ref as ibr  # noqa: E402

RIGHT, ROW_ORDER = 0, 1
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def lib():
    so = hostbuild.build("fpfh_ball_check.cpp", "fpfh_ball_check")
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    so.fbc_cloud.argtypes, so.fbc_cloud.restype = [i32, vp, i32, vp, i32, i32, f64, i32, vp, i32, i32, vp, vp, vp, vp], None
    so.fbc_plan.argtypes, so.fbc_plan.restype = [i32, vp, i32, i32, i32, f64, vp, vp], None
    return so


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_plan(lib, pts, rows, radius):
    """the host build's plan of one cloud at the grid radius of `radius` -> (edges (3,) of the points' dtype, enlarged, flat)"""
    pts = np.ascontiguousarray(pts)
    edges, flags = np.zeros(3), np.zeros(3, np.int32)
    lib.fbc_plan(int(pts.dtype == np.float64), _p(pts), pts.shape[1], pts.shape[0], pts.shape[0] if rows is None else rows, float(radius),
                 _p(edges), _p(flags))
    return edges.astype(pts.dtype), bool(flags[0]), bool(flags[1])


def host(lib, pts, nrm, radius, rows=None, variant=RIGHT, at=None):
    """the header's passes on one cloud -> dict out ((m, 33), or (q, 33) with at), cnt (m, 33) int64, order, stats"""
    pts, nrm = np.ascontiguousarray(pts), np.ascontiguousarray(nrm)
    assert nrm.dtype == pts.dtype
    m = pts.shape[0]
    at = None if at is None else np.ascontiguousarray(at)
    q = 0 if at is None else at.size
    out = np.full((m if at is None else q, fr.CH), np.nan, pts.dtype)
    cnt, order, stats = np.full((m, fr.CH), -7, np.int32), np.zeros(m, np.int64), np.zeros(5, np.int64)
    lib.fbc_cloud(int(pts.dtype == np.float64), _p(pts), pts.shape[1], _p(nrm), m, m if rows is None else rows, float(radius), variant, _p(at),
                  int(at is not None and at.dtype == np.int64), q, _p(out), _p(cnt), _p(order), _p(stats))
    return dict(out=out, cnt=cnt.astype(np.int64), order=order[order >= 0], stats=stats)


def ref(lib, pts, nrm, radius, rows=None, **kw):
    """the numpy restatement, with the plan of the host build where the layout needs one"""
    plan = host_plan(lib, pts, rows, radius)
    return fbr.fpfh_ball_ref(pts, nrm, radius, rows, plan=plan if (plan[1] or plan[2]) else None, **kw), plan


def same(got, want):
    return fr.same_bits(got["cnt"], want["cnt"]) and fr.same_bits(got["out"], want["out"])


# ------------------------------------------------------------------ the reference against tests/fpfh_ref.py
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_reference_is_fpfh_ref_on_a_full_width_index(dtype):
    """wherever every count is <= 255: out equals fpfh_ref on the full-width index in grid order bit for bit, the counts its uint8 counts"""
    for m, rows, members in ((300, None, 40), (300, 211, 4), (65, None, 12), (300, None, 150)):
        P, Nn = fbc.cloud(7 + m + members, m, dtype, dead=True)
        r = ibc.ball_radius(P[:rows], members)
        got = fbr.fpfh_ball_ref(P, Nn, r, rows)
        full = ibr.full_index(ibr.grid_order(P, rows, r), m)
        out, cnt = fr.fpfh_ref(P, Nn, full, rows, r)
        assert got["cnt"].max() <= 255 and (members < 40 or got["cnt"][:, :fr.BINS].sum(axis=1).max() > 32)       # (beyond the k-slot form)
        assert fr.same_bits(got["out"], out) and np.array_equal(got["cnt"], cnt.astype(np.int64))


# ------------------------------------------------------------------ the header against the reference
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,rows,members,cols", [(300, None, 4, 3), (300, 211, 40, 6), (65, None, 12, 3), (300, None, 150, 6), (40, 33, 8, 3),
                                                 (2, None, 1, 3), (1, None, 1, 3)])
def test_random_clouds(lib, dtype, m, rows, members, cols):
    P, Nn = fbc.cloud(m + members, m, dtype, cols=cols, dead=m >= 40)
    r = ibc.ball_radius(P[:rows], members) if m > 2 else 5.0
    want, plan = ref(lib, P, Nn, r, rows)
    got = host(lib, P, Nn, r, rows)
    assert not plan[1] and not plan[2]
    assert fr.same_bits(got["order"], want["order"])
    assert same(got, want)
    pairs = want["cnt"][:, :fr.BINS].sum(axis=1)
    assert (want["cnt"][:, fr.BINS:2 * fr.BINS].sum(axis=1) == pairs).all() and (want["cnt"][:, 2 * fr.BINS:].sum(axis=1) == pairs).all()
    if m >= 65:
        assert abs(np.median(pairs[pairs > 0]) - members) <= max(2, 0.5 * members)                 # (the ball holds what the case says)
        assert (members >= 40) == (pairs.max() > 31)
    if m >= 40:
        for i in fbc.DEAD_ROWS:
            assert not want["cnt"][i].any() and not want["out"][i].any()
    if rows is not None:
        assert not want["cnt"][rows:].any() and not want["out"][rows:].any()
    if m == 2:
        assert (pairs == 1).all() and (want["out"].reshape(2, 3, 11).sum(-1) == 200.0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_dead_rows(lib, dtype):
    """a NaN coordinate, an inf coordinate, a zero normal, a NaN normal, an exact duplicate: the dead rows get zeros and enter no other
    row's counts; the duplicates are not near each other (FPFH's rule, unlike ISS's members) and, with equal normals, have equal rows"""
    P, Nn = fbc.cloud(3, 120, dtype, dead=True)
    Nn[11] = Nn[10]
    r = ibc.ball_radius(P, 25)
    want, _ = ref(lib, P, Nn, r)
    assert same(host(lib, P, Nn, r), want)
    for i in fbc.DEAD_ROWS:
        assert not want["cnt"][i].any() and not want["out"][i].any()
    assert want["cnt"][10].any() and np.array_equal(want["cnt"][10], want["cnt"][11]) and fr.same_bits(want["out"][10], want["out"][11])
    alive = np.ones(120, bool)
    alive[list(fbc.DEAD_ROWS)] = False
    Q, Mn = P[alive], Nn[alive]
    sub = fbr.fpfh_ball_ref(Q, Mn, r)
    assert np.array_equal(sub["cnt"], want["cnt"][alive])                                      # the dead rows entered nothing


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["bin_centres", "clamp", "theta_pi", "tie", "parallel", "dead_rows"])
def test_designed_pairs(lib, dtype, name):
    """the designed FPFH pairs of tests/fpfh_cases.py with a radius that holds the whole cloud"""
    c = fc.designed(dtype)[name]
    want, _ = ref(lib, c["points"], c["normals"], 1000.0, c["rows"])
    assert same(host(lib, c["points"], c["normals"], 1000.0, c["rows"]), want)
    assert want["cnt"].any()
    if name == "tie":
        assert (want["cnt"].sum(axis=1) == 3).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_cloud_with_no_live_rows(lib, dtype):
    P, Nn = fbc.cloud(1, 12, dtype)
    got = host(lib, P, Nn, 0.5, rows=0)
    assert not got["cnt"].any() and not got["out"].any() and got["order"].size == 0
    assert same(got, fbr.fpfh_ball_ref(P, Nn, 0.5, 0))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ibc.LAYOUT_NAMES)
def test_layouts(lib, dtype, name):
    """every layout of the coverage claim with seeded unit normals: the plan comes from the host build where a grid was enlarged or flat"""
    P, r1, _ = ibc.layouts(dtype)[name]
    Nn = fbc.normals(41, P.shape[0], dtype)
    want, plan = ref(lib, P, Nn, r1)
    got = host(lib, P, Nn, r1)
    assert (plan[1] or plan[2]) == (name in ("two clusters", "far outlier", "flat"))
    assert fr.same_bits(got["order"], want["order"])
    assert same(got, want)
    mem = ibr.members_brute(P, None, r1)
    Q = P.astype(np.float64)
    apart = ((Q[:, None, :] - Q[None, :, :]) ** 2).sum(-1) > 0
    assert np.array_equal(want["cnt"][:, :fr.BINS].sum(axis=1), (mem & apart).sum(axis=1))     # (random normals: every near row is a pair)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_wide_count(lib, dtype):
    """a 20 x 20 unit lattice in z = 0 with normals +z and radius 100: every one of a row's 399 pairs falls in theta-bin 5, alpha-bin 16,
    phi-bin 27, so three counters hold 399 and out is 200 there -- a byte counter would hold 399 - 256 = 143"""
    P, Nn = fbc.wide_lattice(dtype)
    want = fbr.fpfh_ball_ref(P, Nn, fbc.WIDE_RADIUS)
    expect = np.zeros((400, fr.CH), np.int64)
    expect[:, list(fbc.WIDE_CHANNELS)] = 399
    assert np.array_equal(want["cnt"], expect)
    assert (want["out"] == np.where(expect > 0, 200.0, 0.0)).all()
    assert same(host(lib, P, Nn, fbc.WIDE_RADIUS), want)
    assert 399 - 256 == 143 and (expect.astype(np.uint8).max() == 143)


def test_refuses_a_near_list_in_row_order(lib):
    """(float64: rounded to float32 the two orders give the same outputs on such a cloud)"""
    dtype = np.float64
    P = ibc.cube(5, 300, dtype)
    Nn = fbc.normals(5, 300, dtype)
    r = ibc.ball_radius(P, 40)
    right, wrong = fbr.fpfh_ball_ref(P, Nn, r), fbr.fpfh_ball_ref(P, Nn, r, row_order=True)
    assert same(host(lib, P, Nn, r), right)
    assert np.array_equal(wrong["cnt"], right["cnt"])
    differ = (wrong["out"] != right["out"]).any(axis=1)
    print("rows whose out differs between the two orders: %d of 300" % differ.sum())
    assert differ.sum() >= 285                                                                 # (nearly every row: 298 here)
    got = host(lib, P, Nn, r, variant=ROW_ORDER)
    assert same(got, wrong) and not same(got, right)
    assert np.allclose(wrong["out"], right["out"], rtol=1e-12, atol=1e-12)                     # (the same rows: only the order of the sum differs)


# ------------------------------------------------------------------ at
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("itype", [np.int32, np.int64])
def test_at(lib, dtype, itype):
    m, rows = 90, 71
    P, Nn = fbc.cloud(77, m, dtype, dead=True)
    r = ibc.ball_radius(P[:rows], 20)
    full = host(lib, P, Nn, r, rows)
    assert same(full, fbr.fpfh_ball_ref(P, Nn, r, rows))
    got = host(lib, P, Nn, r, rows, at=np.arange(m, dtype=itype))
    assert fr.same_bits(got["out"], full["out"]) and fr.same_bits(got["cnt"], full["cnt"])     # arange: the full form; cnt covers every row
    at = fbc.at_entries(m, rows, itype)
    got = host(lib, P, Nn, r, rows, at=at)
    want = fbr.at_ref(full["out"], at, rows)
    assert got["out"].shape == (at.size, fr.CH) and fr.same_bits(got["out"], want) and fr.same_bits(got["cnt"], full["cnt"])
    live = (at.astype(np.int64) >= 0) & (at.astype(np.int64) < rows)
    assert want[live].any() and not want[~live].any() and (~live).sum() >= 5


# ------------------------------------------------------------------ the bound of the GPU cross-check, on the two references alone
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", [31, 32])
def test_cross_check_bound(dtype, seed):
    """test_gpu_fpfh_ball.py compares the whole-ball form with compute_fpfh(k=32) where every ball fits 32 slots, under the bound derived
    in its docstring (fbc.cross_bound).  Here the two numpy references: equal counts on every row, outputs within the bound."""
    P, r = ibc.cross_scene(seed, dtype)
    Nn = fbc.normals(seed, P.shape[0], dtype)
    _, knn = fr.knn_self(P, ibc.K)
    out_k, cnt_k = fr.fpfh_ref(P, Nn, knn, None, r)
    ball = fbr.fpfh_ball_ref(P, Nn, r)
    assert np.array_equal(ball["cnt"], cnt_k.astype(np.int64))
    pairs = ball["cnt"][:, :fr.BINS].sum(axis=1)
    assert pairs.max() <= ibc.K - 1 and pairs.max() > 16 and np.median(pairs) >= 8
    assert np.array_equal(pairs, ibr.members_brute(P, None, r).sum(axis=1))                    # every row within the radius is a pair: n counts the terms
    bound = fbc.cross_bound(int(pairs.max()), dtype)
    diff = np.abs(out_k.astype(np.float64) - ball["out"].astype(np.float64)).max()
    print("seed %d %s: |out difference| max %.3g, bound %.3g" % (seed, np.dtype(dtype).name, diff, bound))
    assert diff <= bound
