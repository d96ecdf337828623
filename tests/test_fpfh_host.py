"""CPU checks of the FPFH descriptor (dicp_amd/fpfh.py) that need no GPU.

``dicp_amd/csrc/dicp_fpfh.h`` -- the rules the HIP kernels execute -- is compiled with g++ through tests/hostcheck/fpfh_check.cpp and held
to tests/fpfh_ref.py: the bin counts integer for integer, the descriptor bit for bit, on random clouds (both dtypes, both index dtypes,
ragged, with a radius) and on the designed ones; the same comparison is shown to refuse five wrong rules.  The half-plane rule of the
theta bin is held to the atan2 form, and the descriptor to its invariance under a rigid motion.

About the wrong rule "self not skipped": a slot at distance 0 is never near (r2 > 0), so `j != i` alone decides nothing; the wrong rule of
variant 3 drops both tests, as an implementation that forgot about the row itself would.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostbuild  # noqa: E402
import fpfh_cases as fc  # noqa: E402
import fpfh_ref as fr  # noqa: E402

RIGHT, TIE_SWAP, STRICT_EDGE, KEEP_SELF, SEARCH_D2, NORM_K = range(6)
DTYPES = [np.float32, np.float64]
ITYPES = [np.int64, np.int32]


@pytest.fixture(scope="module")
def lib():
    so = hostbuild.build("fpfh_check.cpp", "fpfh_check")
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    so.fpc_constants.argtypes, so.fpc_constants.restype = [vp], None
    so.fpc_bins.argtypes, so.fpc_bins.restype = [vp, vp, vp, i32, vp, vp], None
    so.fpc_cloud.argtypes, so.fpc_cloud.restype = [i32, i32, vp, i32, vp, vp, vp, i32, i32, i32, f64, i32, vp, vp], None
    return so


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host(lib, c, radius=None, variant=RIGHT, itype=np.int64, d2=None):
    """the header's two passes on one cloud (a dict of fpfh_cases) -> (out, cnt)"""
    pts, nrm = np.ascontiguousarray(c["points"]), np.ascontiguousarray(c["normals"])
    idx = np.ascontiguousarray(fc.index_dtype(c["idx"], itype))
    m, k = idx.shape
    sd2 = np.ascontiguousarray((np.ones((m, k)) if d2 is None else d2).astype(pts.dtype))
    cnt, out = np.zeros((m, 33), np.uint8), np.zeros((m, 33), pts.dtype)
    lib.fpc_cloud(int(pts.dtype == np.float64), int(itype == np.int64), _p(pts), pts.shape[1], _p(nrm), _p(idx), _p(sd2), m, c["rows"], k,
                  0.0 if radius is None else float(radius), variant, _p(cnt), _p(out))
    return out, cnt


def ref(c, radius=None, itype=np.int64, **kw):
    return fr.fpfh_ref(c["points"], c["normals"], fc.index_dtype(c["idx"], itype), c["rows"], radius, **kw)


def same(got, want):
    return np.array_equal(got[1], want[1]) and fr.same_bits(got[0], want[0])


# ------------------------------------------------------------------ the header against the reference
def test_constants(lib):
    c = np.zeros(5, np.int32)
    lib.fpc_constants(_p(c))
    assert list(c) == [fr.BINS, fr.CH, 1, 32, 48]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("m,k,rows,radius,cols", [(300, 8, None, None, 3), (300, 16, 211, 0.45, 4), (65, 32, None, None, 3), (40, 1, 33, None, 6),
                                                  (2, 3, None, None, 3), (1, 2, None, None, 3), (500, 31, None, 0.3, 3)])
def test_random_clouds(lib, dtype, itype, m, k, rows, radius, cols):
    c = fc.random_cloud(m + k, m, k, dtype, rows=rows, cols=cols, planar=(k == 16))
    want = ref(c, radius, itype)
    if m >= 40 and k >= 2:                                                      # (k = 1: the one neighbour is the row itself)
        assert want[1].sum() > 0 and (want[1].sum(axis=1) == 0).any()          # pairs, and rows without any
    assert same(host(lib, c, radius, itype=itype), want)
    live = want[0][want[1].sum(axis=1) > 0].astype(np.float64).reshape(-1, 3, 11).sum(-1)
    assert np.allclose(live, 200.0, rtol=1e-5)                                  # every feature of a row with pairs sums to 100 + 100
    assert not want[0][c["rows"]:].any() and not want[1][c["rows"]:].any()


def test_the_radius_cut_uses_the_recomputed_distance(lib):
    c = fc.random_cloud(5, 200, 16, np.float64, garbage=False)
    all_, cut = ref(c), ref(c, 0.25)
    assert cut[1].sum() < all_[1].sum() and same(host(lib, c, 0.25), cut)
    far = dict(c, idx=np.where(c["d2"] <= 0.25 * 0.25, c["idx"], -1))             # the slots a ball query would have left out
    assert same(ref(far), cut)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["bin_centres", "clamp", "theta_pi", "tie", "parallel", "dead_rows"])
def test_designed_clouds(lib, dtype, name):
    c = fc.designed(dtype)[name]
    want = ref(c)
    for itype in ITYPES:
        assert same(host(lib, c, itype=itype), want)
    out, cnt = want
    if name == "bin_centres":
        for p in range(33):
            for row in (2 * p, 2 * p + 1):
                assert cnt[row, c["channel"][p]] == 1 and cnt[row].sum() == 3
        assert sorted(set(np.flatnonzero(cnt.sum(axis=0)))) == list(range(33))    # every bin of every feature is reached
    if name == "clamp":
        assert list(cnt[:, 11:22].argmax(axis=1)) == [10, 10, 0, 0]
    if name == "theta_pi":
        P, Nn = c["points"].astype(np.float64), c["normals"].astype(np.float64)
        f = fr.pair_features(P[0::2], Nn[0::2], P[1::2], Nn[1::2])
        assert (f["cos"] == -1.0).all() and (f["sin"] == 0.0).all() and np.signbit(f["sin"]).any() and not np.signbit(f["sin"]).all()
        assert (cnt[:, :11].argmax(axis=1) == 10).all()                           # the closed end: pi belongs to the last bin, whatever the zero's sign
    if name == "tie":
        assert list(np.flatnonzero(cnt[0])) == [8, 16, 30] and list(np.flatnonzero(cnt[1])) == [2, 16, 24]       # phi = +0.6 from either side
    if name == "parallel":
        assert list(cnt.sum(axis=1)) == [0, 3, 3]                                 # rows 0 and 1 have no frame between them
        assert out[0].astype(np.float64).sum() == pytest.approx(300.0)
        s1 = 100.0 * cnt[1].astype(np.float64) / 1.0                             # (row 1 has one pair)
        assert np.allclose(out[0].astype(np.float64), s1)                        # row 0: no SPFH of its own, row 1's through the weight
    if name == "dead_rows":
        assert list(cnt.sum(axis=1)) == [3, 3, 0, 0, 0, 0, 18, 18, 6, 3]
        assert not out[2:6].any()                                                 # zero / NaN / inf normals, a NaN coordinate: 33 zeros
        assert np.isfinite(out).all()


# ------------------------------------------------------------------ the comparison refuses wrong rules
def refuses(lib, c, variant, radius=None, d2=None, **kw):
    right, wrong = ref(c, radius), ref(c, radius, **kw)
    got = host(lib, c, radius, variant=variant, d2=d2)
    assert same(host(lib, c, radius), right)
    assert not same(wrong, right)
    assert same(got, wrong) and not same(got, right)
    return right, wrong


def test_refuses_a_swap_on_ties(lib):
    right, wrong = refuses(lib, fc.designed(np.float64)["tie"], TIE_SWAP, tie_swap=True)
    assert list(np.flatnonzero(wrong[1][0])) == [2, 16, 24]                       # phi = -0.6
    c = fc.random_cloud(1, 300, 8, np.float32)                                    # (no pair of a random cloud is a tie)
    assert same(host(lib, c, variant=TIE_SWAP), ref(c))


def test_refuses_a_strict_edge_test(lib):
    right, wrong = refuses(lib, fc.designed(np.float64)["theta_pi"], STRICT_EDGE, strict_edge=True)
    assert (right[1][:, :11].argmax(axis=1) == 10).all() and (wrong[1][:, :11].argmax(axis=1) == 5).all()
    c = fc.random_cloud(1, 300, 8, np.float64)                                    # (no pair of a random cloud sits on sin = 0)
    assert same(host(lib, c, variant=STRICT_EDGE), ref(c))


def test_refuses_a_row_that_is_its_own_neighbour(lib):
    c = fc.random_cloud(2, 120, 8, np.float64, garbage=False)                     # every row finds itself in slot 0
    assert (c["idx"][:, 0] == np.arange(120)).all()
    right, wrong = refuses(lib, c, KEEP_SELF, keep_self=True)
    assert np.isfinite(right[0]).all() and np.isnan(wrong[0]).any()               # the weight 1 / 0
    refuses(lib, fc.designed(np.float64)["dead_rows"], KEEP_SELF, keep_self=True)


def test_refuses_the_distance_of_the_search(lib):
    c = fc.random_cloud(3, 200, 12, np.float32, garbage=False)
    d2 = c["d2"].astype(np.float64)
    d2[~np.isfinite(d2)] = 1.0
    right, wrong = refuses(lib, c, SEARCH_D2, d2=d2, search_d2=d2.astype(np.float32))
    assert np.array_equal(right[1], wrong[1])                                     # the counts are the same ...
    assert np.allclose(right[0], wrong[0], rtol=1e-4, atol=1e-3)                  # ... the weights differ in float32's last bits


def test_refuses_counts_divided_by_k(lib):
    c = fc.random_cloud(4, 200, 12, np.float64)
    right, wrong = refuses(lib, c, NORM_K, norm_k=True)
    assert np.array_equal(right[1], wrong[1])
    assert (wrong[0].sum(axis=1) <= right[0].sum(axis=1) + 1e-9).all()


# ------------------------------------------------------------------ the theta rule against atan2
def test_theta_rule_is_the_atan2_bin(lib):
    rng = np.random.default_rng(0)
    n = 200000
    P = rng.uniform(-1, 1, (2, n, 3))
    Nn = fc.unit(rng.standard_normal((2, n, 3)))
    f = fr.pair_features(P[0], Nn[0], P[1], Nn[1])
    c, s = np.ascontiguousarray(f["cos"]), np.ascontiguousarray(f["sin"])
    want, dist = fr.bin_theta_atan2(c, s)
    clear = f["frame"] & (dist > 1e-9)
    assert clear.sum() > 0.999 * n
    theta, unit = np.zeros(n, np.int32), np.zeros(n, np.int32)
    a = np.ascontiguousarray(f["alpha"])
    lib.fpc_bins(_p(c), _p(s), _p(a), n, _p(theta), _p(unit))
    assert np.array_equal(theta[clear], want[clear]) and np.array_equal(fr.bin_theta(c, s)[clear], want[clear])
    assert sorted(set(want[clear])) == list(range(11))
    assert np.array_equal(unit, np.clip(np.floor(11.0 * ((a + 1.0) * 0.5)), 0, 10).astype(np.int32)) and np.array_equal(unit, fr.bin_unit(a))
    # the unit circle sampled densely, every edge from both sides
    t = np.linspace(-np.pi, np.pi, 100001)[1:]
    c, s = np.cos(t), np.sin(t)
    want, dist = fr.bin_theta_atan2(c, s)
    theta = np.zeros(t.size, np.int32)
    lib.fpc_bins(_p(c), _p(s), _p(c), t.size, _p(theta), _p(np.zeros(t.size, np.int32)))
    assert np.array_equal(theta[dist > 1e-9], want[dist > 1e-9])
    # NaN features: bin 0 (alpha, phi), never out of range
    bad = np.array([np.nan, np.inf, -np.inf, 1.0, -1.0, 1.0000001, -1.0000001])
    theta, unit = np.zeros(7, np.int32), np.zeros(7, np.int32)
    lib.fpc_bins(_p(bad), _p(bad), _p(bad), 7, _p(theta), _p(unit))
    assert list(unit) == [0, 10, 0, 10, 0, 10, 0] and ((theta >= 0) & (theta <= 10)).all()


# ------------------------------------------------------------------ invariance
def test_descriptors_survive_a_rigid_motion():
    """float64, m = 1500, k = 24, radius 0.6: a rigidly moved, row-permuted copy with its normals moved along (what the moved viewpoint
    gives) has, for at least 99 % of its rows, the row it came from as the nearest descriptor."""
    m, k, radius = 1500, 24, 0.6
    P = fc.scene(0, m)
    Nn = fc.normals_np(P, 16, fc.VIEWPOINT)
    mv = fc.moved_copy(P, seed=0)
    X, Nx = mv["x"], Nn[mv["src"]] @ mv["R"].T
    assert ((fc.VIEWPOINT @ mv["R"].T + mv["t"] - X) * Nx).sum(-1).min() > 0         # they face the moved viewpoint
    f0, _ = fr.fpfh_ref(P, Nn, fr.knn_self(P, k)[1], radius=radius)
    f1, _ = fr.fpfh_ref(X, Nx, fr.knn_self(X, k)[1], radius=radius)
    to, _ = fc.nearest_rows(f1, f0)
    share = float((to == mv["src"]).mean())
    print("rows whose nearest descriptor is the row they came from: %.4f" % share)
    assert share >= 0.99
