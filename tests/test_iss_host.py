"""CPU checks of the ISS keypoints (dicp_amd/iss.py) that need no GPU.

``dicp_amd/csrc/dicp_iss.h`` -- the rules the HIP kernels execute -- is compiled with g++ through tests/hostcheck/iss_check.cpp and held to
tests/iss_ref.py: eigenvalues, saliency and counts bit for bit, the keypoint mask exactly, on random clouds (both dtypes, both index
dtypes, ragged, with radii, a second index for the suppression) and on the designed ones; the same comparison is shown to refuse wrong
rules.  The restatement's eigenvalues are held to numpy.linalg.eigvalsh within B u trace, and its saliency decisions to the same rule on
eigvalsh's eigenvalues.

About the sweeps.  ISS_SWEEPS = 6 is the number after which every off-diagonal entry is EXACTLY 0 on all the families here (about half of
the neighbourhoods need the sixth sweep for that, none a seventh): test_six_sweeps_reach_exact_zeros holds the worked matrix after 5 and
after 6 sweeps to the restatement and shows the comparison to refuse 5.  The three eigenvalues themselves stop changing earlier -- on
none of two million sampled matrices (random, graded over 16 decades, near-identity, two close eigenvalues: scripts/iss_edges.py,
profiles/r31_iss_edges.txt) did a sweep after the fourth change a bit of them -- so at the level of a cloud's outputs a fifth sweep in
place of six cannot be told apart, and the wrong variant of test_refuses_too_few_sweeps runs 2 sweeps.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostbuild  # noqa: E402
import iss_cases as ic  # noqa: E402
import iss_ref as ir  # noqa: E402

RIGHT, FEW_SWEEPS, GAMMA_LE, TIE_BOTH, SELF_TWICE, NMS_NO_RADIUS = range(6)
DTYPES = [np.float32, np.float64]
ITYPES = [np.int64, np.int32]
B_BOUND = 27.5                      # twice the largest B seen over the families, 13.72 (profiles/r31_iss_edges.txt), rounded up


@pytest.fixture(scope="module")
def lib():
    so = hostbuild.build("iss_check.cpp", "iss_check")
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    so.isc_constants.argtypes, so.isc_constants.restype = [vp], None
    so.isc_eigenvalues.argtypes, so.isc_eigenvalues.restype = [vp, i32, i32, vp, vp], None
    so.isc_cloud.argtypes = [i32, i32, vp, i32, vp, i32, vp, i32, i32, i32, f64, f64, f64, f64, i32, i32, i32, vp, vp, vp, vp]
    so.isc_cloud.restype = None
    return so


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host(lib, c, r1=None, r2=None, gamma21=0.975, gamma32=0.975, min_neighbors=5, variant=RIGHT, sweeps=ir.SWEEPS, itype=np.int64, nms=None):
    """the header's two passes on one cloud (a dict of iss_cases) -> dict eig, sal, count, mask"""
    pts = np.ascontiguousarray(c["points"])
    idx = np.ascontiguousarray(ic.index_dtype(c["idx"], itype))
    nms = idx if nms is None else np.ascontiguousarray(ic.index_dtype(nms, itype))
    m, k = idx.shape
    eig, sal = np.zeros((m, 3), pts.dtype), np.zeros(m, pts.dtype)
    cnt, mask = np.zeros(m, np.int32), np.zeros(m, np.uint8)
    lib.isc_cloud(int(pts.dtype == np.float64), int(itype == np.int64), _p(pts), pts.shape[1], _p(idx), k, _p(nms), nms.shape[1], m, c["rows"],
                  0.0 if r1 is None else float(r1), 0.0 if r2 is None else float(r2), gamma21, gamma32, min_neighbors, variant, sweeps,
                  _p(eig), _p(sal), _p(cnt), _p(mask))
    return dict(eig=eig, sal=sal, count=cnt, mask=mask.astype(bool))


def ref(c, r1=None, r2=None, itype=np.int64, nms=None, **kw):
    return ir.keypoints_ref(c["points"], ic.index_dtype(c["idx"], itype), c["rows"], r1, r2,
                            nms_idx=None if nms is None else ic.index_dtype(nms, itype), **kw)


def host_eigenvalues(lib, a, sweeps):
    A = np.ascontiguousarray(np.stack(a, axis=-1))
    lam, worked = np.zeros((A.shape[0], 3)), np.zeros((A.shape[0], 6))
    lib.isc_eigenvalues(_p(A), A.shape[0], sweeps, _p(lam), _p(worked))
    return lam, worked


# ------------------------------------------------------------------ the header against the reference
def test_constants(lib):
    c = np.zeros(3, np.int32)
    lib.isc_constants(_p(c))
    assert list(c) == [ir.SWEEPS, 1, 32]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("m,k,rows,cut,cols", [(300, 8, None, None, 3), (300, 16, 211, 0.5, 4), (65, 32, None, None, 3), (40, 1, 33, None, 6),
                                              (2, 3, None, None, 3), (1, 2, None, None, 3), (500, 31, None, 0.7, 3), (200, 12, 150, 0.0, 3)])
def test_random_clouds(lib, dtype, itype, m, k, rows, cut, cols):
    c = ic.random_cloud(m + k, m, k, dtype, rows=rows, cols=cols, planar=(k == 16))
    r1 = None if cut is None else (1e-6 if cut == 0.0 else ic.median_radius(c, cut))         # (1e-6: cuts every slot but the duplicates)
    r2 = None if r1 is None else 0.8 * r1
    want = ref(c, r1, r2, itype)
    if m >= 200 and k >= 8 and cut != 0.0:
        assert (want["sal64"] > 0).sum() > 10 and want["mask"].sum() >= 2 and (want["sal64"][:c["rows"]] == 0).any()
        assert want["mask"].sum() < (want["sal64"] > 0).sum()                   # (the suppression suppresses)
    if cut == 0.0:
        assert want["count"].max() == 2 and not want["mask"].any()            # the duplicate pair alone survives the cut
    assert ir.same(host(lib, c, r1, r2, itype=itype), want)
    assert not want["sal"][c["rows"]:].any() and not want["count"][c["rows"]:].any() and not want["mask"][c["rows"]:].any()
    assert (np.diff(want["eig"].astype(np.float64), axis=1) >= 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_second_index_for_the_suppression(lib, dtype):
    c = ic.random_cloud(7, 300, 12, dtype)
    nms = ic.random_cloud(7, 300, 20, dtype)["idx"]
    r = ic.median_radius(c, 0.8)
    want, plain = ref(c, r, r, nms=nms), ref(c, r, r)
    assert ir.same(host(lib, c, r, r, nms=nms), want)
    assert ir.same_bits(want["sal"], plain["sal"]) and want["mask"].sum() < plain["mask"].sum()       # more members: fewer maxima


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["duplicates", "planar", "collinear", "counts", "ratio", "only_itself", "non_finite"])
def test_designed_clouds(lib, dtype, name):
    c = ic.designed(dtype)[name]
    want = ref(c, **c["params"])
    for itype in ITYPES:
        assert ir.same(host(lib, c, itype=itype, **c["params"]), want)
    sal, cnt, mask, eig = want["sal64"], want["count"], want["mask"], want["eig"].astype(np.float64)
    if name == "duplicates":
        assert sal[0] > 0 and sal[0] == sal[1] and list(cnt[:3]) == [10, 10, 1] and list(np.flatnonzero(mask)) == [0]
    if name == "planar":
        assert eig[0, 0] == 0.0 and eig[0, 1] > 0 and not sal.any() and not mask.any() and cnt[0] == 8
    if name == "collinear":
        assert eig[0, 0] == 0.0 and eig[0, 1] == 0.0 and eig[0, 2] > 0 and not sal.any() and not mask.any()
    if name == "counts":
        assert list(cnt[[0, 5]]) == [5, 4] and sal[0] > 0 and sal[5] == 0 and list(np.flatnonzero(mask)) == [0]
        four = ref(c, min_neighbors=4)
        assert four["sal64"][5] > 0 and list(np.flatnonzero(four["mask"])) == [0, 5]        # one below: the count alone decided
        assert ir.same(host(lib, c, min_neighbors=4), four)
    if name == "ratio":
        assert eig[0, 1] == 0.25 * eig[0, 2] and eig[0, 0] == 0.25 * eig[0, 1] and sal[0] > 0     # (at the default gammas it is salient)
        for g21, g32, salient in ((0.25, 0.5, False), (0.5, 0.25, False), (0.5, 0.5, True), (0.25, 0.25, False)):
            at = ref(c, gamma21=g21, gamma32=g32)
            assert bool(at["sal64"][0] > 0) == salient and bool(at["mask"][0]) == salient
            assert ir.same(host(lib, c, gamma21=g21, gamma32=g32), at)
    if name == "only_itself":
        assert list(cnt) == [1, 1, 0, 0, 0, 0] and not eig.any() and not sal.any() and not mask.any()
    if name == "non_finite":
        clean = ic.non_finite(dtype)[1]
        alone = ref(clean)
        assert cnt[0] == 9 and sal[0] > 0 and sal[0] == alone["sal64"][0] and mask[0] and list(cnt[9:]) == [0, 0]


# ------------------------------------------------------------------ the comparison refuses wrong rules
def refuses(lib, c, variant, r1=None, r2=None, host_sweeps=ir.SWEEPS, nms=None, params=None, **kw):
    params = params or {}
    right, wrong = ref(c, r1, r2, nms=nms, **params), ref(c, r1, r2, nms=nms, **dict(params, **kw))
    got = host(lib, c, r1, r2, variant=variant, sweeps=host_sweeps, nms=nms, **params)
    assert ir.same(host(lib, c, r1, r2, nms=nms, **params), right)
    assert not ir.same(wrong, right)
    assert ir.same(got, wrong) and not ir.same(got, right)
    return right, wrong


def test_six_sweeps_reach_exact_zeros(lib):
    """the worked matrix after 5 sweeps is refused where 6 are needed: its off-diagonals are not yet exactly 0"""
    a, _, _ = ic.family_covariances("uniform", 4000, 3)
    lam6, needed, w6 = ir.eigenvalues(a, 6, return_needed=True, return_worked=True)
    lam5, w5 = ir.eigenvalues(a, 5, return_worked=True)
    assert (needed == 6).sum() > 1000 and needed.max() == 6                    # many need the sixth sweep, none a seventh
    assert not w6[:, [1, 2, 4]].any() and w5[needed == 6][:, [1, 2, 4]].any(axis=1).all()
    h6, h5 = host_eigenvalues(lib, a, 6), host_eigenvalues(lib, a, 5)
    assert ir.same_bits(h6[0], lam6) and ir.same_bits(h6[1], w6)
    assert ir.same_bits(h5[1], w5) and not ir.same_bits(h5[1], w6)             # five sweeps: refused
    assert ir.same_bits(host_eigenvalues(lib, a, 7)[1], w6)                    # a seventh changes nothing
    assert ir.same_bits(lam5, lam6)                                            # (the eigenvalues had settled: see the module's docstring)


def test_refuses_too_few_sweeps(lib):
    c = ic.random_cloud(3, 300, 12, np.float64, garbage=False)
    right, wrong = refuses(lib, c, FEW_SWEEPS, host_sweeps=2, sweeps=2)
    assert np.allclose(right["eig"], wrong["eig"], rtol=0, atol=1e-3)


def test_refuses_a_loose_gamma_test(lib):
    c = ic.designed(np.float64)["ratio"]
    for g21, g32 in ((0.25, 0.5), (0.5, 0.25)):
        right, wrong = refuses(lib, c, GAMMA_LE, params=dict(gamma21=g21, gamma32=g32), gamma_le=True)
        assert right["sal64"][0] == 0 and wrong["sal64"][0] > 0 and wrong["mask"][0]
    r = ic.random_cloud(1, 300, 8, np.float32)                                  # (no row of a random cloud sits on a gamma)
    assert ir.same(host(lib, r, variant=GAMMA_LE), ref(r))


def test_refuses_a_tie_kept_on_both_sides(lib):
    right, wrong = refuses(lib, ic.designed(np.float64)["duplicates"], TIE_BOTH, tie_both=True)
    assert list(np.flatnonzero(right["mask"])) == [0] and list(np.flatnonzero(wrong["mask"])) == [0, 1]


def test_refuses_a_row_counted_twice(lib):
    c = ic.random_cloud(2, 120, 8, np.float64, garbage=False)                   # every row finds itself in slot 0
    assert (c["idx"][:, 0] == np.arange(120)).all()
    right, wrong = refuses(lib, c, SELF_TWICE, self_twice=True)
    assert (wrong["count"] == right["count"] + 1).all() and not np.array_equal(wrong["eig"], right["eig"])


def test_refuses_a_suppression_without_its_radius(lib):
    c = ic.random_cloud(5, 300, 16, np.float64, garbage=False)
    r = ic.median_radius(c, 0.9)
    right, wrong = refuses(lib, c, NMS_NO_RADIUS, r, 0.5 * r, no_radius=True, params=dict(min_neighbors=3))
    assert ir.same_bits(right["sal"], wrong["sal"]) and wrong["mask"].sum() < right["mask"].sum()


# ------------------------------------------------------------------ accuracy
def test_eigenvalues_against_eigvalsh(lib):
    """The restatement's eigenvalues against numpy.linalg.eigvalsh in float64 over the families of tests/iss_cases.py (uniform, planar at
    1e-3, linear at 1e-4, clouds 2.5 km from the origin: 12000 neighbourhoods of 12 points each; count = 3: 200): |lambda - eigvalsh| <=
    B u trace with B_BOUND, twice the largest B seen (13.72, the linear family; scripts/iss_edges.py writes them to
    profiles/r31_iss_edges.txt).  Every saliency decision agrees with the same rule on eigvalsh's eigenvalues except on rows whose margin
    (gamma21 l2 - l1, gamma32 l1 - l0, or l0 itself) is within that bound: those are the count = 3 rows, whose l0 is a rounding residue
    of a rank-2 matrix (with their real count, 3 < min_neighbors, the rule says 0 on both sides anyway), and they are 200 of 48200
    rows, under 1 %: the family is kept that small for this cap."""
    acc = ic.accuracy()
    total = excluded = 0
    for name, v in acc.items():
        print("%-24s B = %6.2f   sweeps until exact zeros: %s" % (name, v["B"], [int(x) for x in v["needed"]]))
        assert v["B"] <= B_BOUND and v["needed"][ir.SWEEPS + 1] == 0
        assert ir.same_bits(host_eigenvalues(lib, v["a"], ir.SWEEPS)[0], v["lam"])
        count = v["count"]                                                      # 12, or 3: below min_neighbors, both decide 0
        mine = ir.saliency_rule(v["lam"], count, 0.975, 0.975, 5) > 0
        theirs = ir.saliency_rule(v["ref"], count, 0.975, 0.975, 5) > 0
        bound = B_BOUND * ic.U * v["trace"]
        w = v["ref"]
        margin = np.minimum(np.minimum(np.abs(0.975 * w[:, 2] - w[:, 1]), np.abs(0.975 * w[:, 1] - w[:, 0])), np.abs(w[:, 0]))
        out = margin <= bound
        assert np.array_equal(mine[~out], theirs[~out])
        if name != "count 3":
            assert mine.mean() > 0.9 and (~mine).sum() > 0                     # both decisions occur
        else:
            assert (count == 3).all() and not mine.any() and not theirs.any()
        total, excluded = total + out.size, excluded + int(out.sum())
    print("rows excluded for a margin within the bound: %d of %d" % (excluded, total))
    assert total == 48200 and excluded <= 0.01 * total
