"""CPU checks of ransac_correspondences / correspondence_residuals (dicp_amd/register.py) that need no GPU.

The rules of ``dicp_amd/csrc/dicp_ransac.h`` -- the lines the HIP kernels run -- are compiled with g++ through
tests/hostcheck/ransac_check.cpp, run in a serial loop and held to the numpy restatement tests/ransac_ref.py: the hash and the sampler
integer for integer, the sums in front of the fit, the residual chain, the counts, the choice and the inlier sets bit for bit in both
dtypes; the fit inside the bound of tests/ransac_cases.py against float64 numpy Kabsch.  Every deliberately wrong restatement is shown to
be refused by the same comparisons, the argument checks of the two Python functions run before any device work, and the recovery case of
the GPU test is evaluated on the restatement alone.
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.match import correspondence_residuals, ransac_correspondences

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import match_ref as mr  # noqa: E402
import ransac_cases as rc  # noqa: E402
import ransac_ref as rr  # noqa: E402
from gumbel_ref import mix32  # noqa: E402

DTYPES = [np.float32, np.float64]
same_bits = rc.same_bits


@pytest.fixture(scope="module")
def check():
    return rc.build()


def test_fast_fma64_is_the_exact_one(check):
    rng = np.random.default_rng(2)
    n = 1500
    a = rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)
    b = rng.standard_normal(n)
    p = a * b
    cs = [rng.standard_normal(n), -p, np.nextafter(-p, np.inf), np.nextafter(-p, -np.inf), -p * 2.0 ** 53, -p * 2.0 ** -53, np.zeros(n),
          -p * (1 + 2.0 ** -30)]
    for c in cs:
        got = rr.fma64_fast(a, b, c)
        assert same_bits(got, mr.fma64(a, b, c))
        assert same_bits(got, np.array([check.rc_fma(float(u), float(v), float(w)) for u, v, w in zip(a, b, c)]))
    assert not same_bits(rr.fma64_fast(a, b, cs[2]), a * b + cs[2])                 # a separate product is refused
    e = np.array([0.0, -0.0, 1.5, np.inf, np.nan])
    assert same_bits(rr.fma64_fast(e, e, 0.0), np.array([0.0, 0.0, 2.25, np.inf, np.nan]))


# ------------------------------------------------------------------ the sampler: integers only
def test_hash_is_the_gumbel_hash(check):
    v = np.concatenate((np.arange(70), np.random.default_rng(0).integers(0, 1 << 32, 400), [0xFFFFFFFF])).astype(np.uint64)
    assert [check.rc_mix32(int(t)) for t in v] == [int(t) for t in mix32(v)]
    u = np.empty(3, np.uint32)
    for seed, cloud, h in ((0, 0, 0), (123456789, 7, 65535), (0xFFFFFFFF, 31, 1000), (1 << 40 | 5, 2, 3)):
        check.rc_draws(seed & 0xFFFFFFFF, cloud, h, rc._ptr(u))
        assert [int(t) for t in u] == [int(t) for t in rr.draws(seed, cloud, h + 1)[h]]


P_CASES = (3, 4, 5, 64, 65, (1 << 31) - 1)


def header_positions(check, u, P):
    out = np.empty((len(u), 3), np.int32)
    for k, (u0, u1, u2) in enumerate(u):
        check.rc_positions(int(u0), int(u1), int(u2), P, rc._ptr(out[k]))
    return out


@pytest.mark.parametrize("P", P_CASES)
def test_positions_integer_for_integer(check, P):
    edge = (0, 0xFFFFFFFF)
    forced = [(a, b, c) for a in edge for b in edge for c in edge]
    near = [0, 1, 0x55555555, 0x55555556, 0x7FFFFFFF, 0x80000000, 0xAAAAAAAA, 0xAAAAAAAB, 0xFFFFFFFE, 0xFFFFFFFF]
    forced += [(a, b, c) for a in near for b in near[::3] for c in near]
    u = np.concatenate((np.array(forced, dtype=np.uint64), rr.draws(11, 3, 3000)))
    got = header_positions(check, u, P)
    want = rr.positions(u, P)
    assert np.array_equal(got, want)
    assert got.min() >= 0 and got.max() < P
    assert np.all(got[:, 0] != got[:, 1]) and np.all(got[:, 0] != got[:, 2]) and np.all(got[:, 1] != got[:, 2])
    if P <= 5:                                                  # every position is reached, and from both ends of the draws
        assert set(np.unique(got)) == set(range(P))
    for wrong in ("with_replacement", "mod_instead_of_mulhi"):
        assert not np.array_equal(got, rr.positions(u, P, wrong)), wrong


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", (3, 4, 5, 64, 65))
def test_samples_and_sums(check, dtype, P):
    rng = np.random.default_rng(P)
    pairs = rc.cube_pairs(rng, P, dtype, offset=3.0, noise=0.01)
    pairs = (pairs * 2.0 ** rng.integers(-12, 13, (P, 1))).astype(dtype)     # rows of very different sizes: the double sums round, so their order shows
    smp, sm, _ = rc.header_hypotheses(check, pairs, 400, seed=99, cloud=2)
    want = rr.samples(99, 2, 400, P)
    assert np.array_equal(smp, want)
    assert same_bits(sm, rr.sums(pairs, want))
    assert not same_bits(sm, rr.sums(pairs, want, wrong="order_cab"))
    assert not np.array_equal(smp, rr.samples(99, 3, 400, P)) and not np.array_equal(smp, rr.samples(98, 2, 400, P))


# ------------------------------------------------------------------ the fit, inside the bound
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", (0.0, 2500.0))
def test_fit_against_float64_kabsch(check, dtype, offset):
    rng = np.random.default_rng(5)
    pairs = rc.cube_pairs(rng, 300, dtype, offset, noise=0.01)
    smp, _, poses = rc.header_hypotheses(check, pairs, 3000, seed=1)
    ok, share, wc, wr = rc.poses_hold(poses, pairs, smp)
    print("fit %s offset %g: share %.3f, worst dC / bound %.3g, worst dr / bound %.3g" % (np.dtype(dtype).name, offset, share, wc, wr))
    assert share >= rc.MIN_SHARE
    assert ok
    bad = poses.copy()
    bad[:, :9] = poses[:, [0, 3, 6, 1, 4, 7, 2, 5, 8]]          # the transposed rotation is refused
    assert not rc.poses_hold(bad, pairs, smp)[0]
    C = poses[:, :9].astype(np.float64).reshape(-1, 3, 3)
    assert np.all(np.linalg.det(C) > 0.99)                      # proper rotations, the rank-deficient completion included


def test_degenerate_samples_give_finite_proper_poses(check):
    pairs = rc.cube_pairs(np.random.default_rng(8), 3, np.float64)
    pairs[1] = pairs[0]                                         # duplicate points: a rank-1 covariance
    _, _, poses = rc.header_hypotheses(check, pairs, 8, seed=0)
    assert np.isfinite(poses).all()
    assert np.allclose(np.linalg.det(poses[:, :9].reshape(-1, 3, 3)), 1.0)
    pairs[2] = pairs[0]                                         # all three the same: no covariance at all
    _, _, poses = rc.header_hypotheses(check, pairs, 8, seed=0)
    assert np.isfinite(poses).all()


# ------------------------------------------------------------------ residuals, counts, choice, inlier sets: bit for bit on injected poses
def injected(rng, dtype, P, H):
    """pairs with a true pose and noise near the threshold, poses around the truth, with ties, a NaN and an inf pose"""
    pairs = rc.cube_pairs(rng, P, dtype, offset=1.0, noise=0.02)
    tri = pairs.astype(np.float64)
    truth = rr.kabsch(tri[None, :, :3], tri[None, :, 3:])[0][0]
    poses = (truth[None, :] + 0.01 * rng.standard_normal((H, 12)) * (rng.random((H, 1)) < 0.7)).astype(dtype)
    if H > 8:
        poses[5] = poses[2]
        poses[3, 4] = np.nan
        poses[6, 10] = np.inf
    return pairs, poses


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,H", ((3, 1), (64, 65), (257, 40)))
def test_score_matches_restatement(check, dtype, P, H):
    rng = np.random.default_rng(P + H)
    pairs, poses = injected(rng, dtype, P, H)
    thr = 0.035
    d, counts, best, bc = rc.header_score(check, pairs, poses, thr)
    assert same_bits(d, rr.residuals(poses, pairs[:, :3], pairs[:, 3:]))
    rcounts, rbest, rbc = rr.score(poses, pairs, thr)
    assert np.array_equal(counts, rcounts) and (best, bc) == (rbest, rbc)
    if H > 8:
        assert counts[3] == 0 and counts[6] == 0 and counts[5] == counts[2]
    thr2 = rr.thr2_of(thr, dtype)
    assert np.array_equal(d[best] <= thr2, rr.inlier(rr.residuals(poses[best][None], pairs[:, :3], pairs[:, 3:])[0], thr2))


def test_wrong_restatements_are_refused(check):
    for dtype in DTYPES:
        rng = np.random.default_rng(17)
        pairs, poses = injected(rng, dtype, 200, 64)
        poses[9] = poses[2]
        d, counts, best, bc = rc.header_score(check, pairs, poses, 0.035)
        assert same_bits(d, rr.residuals(poses, pairs[:, :3], pairs[:, 3:]))
        assert not same_bits(d, rr.residuals(poses, pairs[:, :3], pairs[:, 3:], wrong="unfused"))
        # a pair exactly on the threshold is in: take thr2 = one of the d themselves
        h, j = 2, int(np.argsort(d[2])[100])
        t = float(np.sqrt(np.float64(d[h, j])))
        while rr.thr2_of(t, dtype) < d[h, j]:
            t = float(np.nextafter(t, np.inf))
        if rr.thr2_of(t, dtype) == d[h, j]:
            _, c2, b2, bc2 = rc.header_score(check, pairs, poses, t)
            assert np.array_equal(c2, rr.score(poses, pairs, t)[0])
            assert not np.array_equal(c2, rr.score(poses, pairs, t, wrong="strict_less")[0])
        # the tie between h = 2 and h = 9 goes to the lower one
        only = np.full_like(poses, np.nan)
        only[2], only[9] = poses[2], poses[2]
        _, c3, b3, _ = rc.header_score(check, pairs, only, 0.035)
        assert b3 == 2 and rr.score(only, pairs, 0.035)[1] == 2 and rr.score(only, pairs, 0.035, wrong="tie_high")[1] == 9


def test_on_the_threshold_is_in_one_ulp_above_is_out(check):
    for dtype in DTYPES:
        T = dtype
        pose = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], dtype=T)
        thr = 0.25                                              # thr2 = 0.0625 exactly in both dtypes
        e_on = T(0.25)
        e_out = np.nextafter(e_on, T(1))
        pairs = np.zeros((4, 6), dtype=T)
        pairs[0, 3] = -e_on                                     # d = 0.0625 = thr2: in
        pairs[1, 4] = e_out                                     # d one step above: out
        pairs[2, 5] = np.nan                                    # a NaN d: out
        d, counts, best, bc = rc.header_score(check, pairs, pose, thr)
        assert d[0, 0] == T(0.0625) and d[0, 1] > T(0.0625) and np.isnan(d[0, 2]) and d[0, 3] == 0
        assert counts[0] == 2 and rr.score(pose, pairs, thr)[0][0] == 2
        assert rr.score(pose, pairs, thr, wrong="strict_less")[0][0] == 1          # d < thr2 drops the pair on the threshold: refused


def test_live_rule(check):
    for dtype, s in rc.SFX.items():
        f = getattr(check, "rc_live_" + s)
        x, y = np.array([1, 2, 3], dtype=dtype), np.array([4, 5, 6], dtype=dtype)
        assert f(1, 0, rc._ptr(x), rc._ptr(y)) == 1 and f(0, 0, rc._ptr(x), rc._ptr(y)) == 0 and f(1, -1, rc._ptr(x), rc._ptr(y)) == 0
        for k in range(3):
            for bad in (np.nan, np.inf, -np.inf):
                xb, yb = x.copy(), y.copy()
                xb[k] = bad
                yb[k] = bad
                assert f(1, 5, rc._ptr(xb), rc._ptr(y)) == 0 and f(1, 5, rc._ptr(x), rc._ptr(yb)) == 0
    x = np.zeros((5, 3), np.float32)
    y = np.zeros((2, 3), np.float32)
    y[1, 0] = np.nan
    x[3, 2] = np.inf
    assert list(rr.live_mask(x, y, np.array([0, -1, 7, 0, 0]), x_rows=4)) == [True, False, False, False, False]     # (7 clamps to the NaN row)


# ------------------------------------------------------------------ the recovery case, on the restatement alone
@pytest.mark.parametrize("seed", range(5))
def test_recovery_case_on_the_restatement(seed):
    a = rr.recovery_case(seed)
    out = rr.ransac_ref(a["x"], a["y"], a["idx"], 0.05, hypotheses=256, seed=seed, refine=1)
    assert out["inliers"][a["truth"]].all()                     # every true inlier is kept
    err = rr.rotation_error(out["pose"][:9], a["C"])
    print("seed %d: best_count %d, inliers %d of %d true, rotation error %.3g" % (seed, out["best_count"], out["inliers"].sum(), a["truth"].sum(), err))
    assert err < 5e-3
    assert out["best_count"] <= out["inliers"].sum()
    plain = rr.kabsch(a["x"], a["y"][a["idx"]])[0]
    assert rr.rotation_error(plain[:9], a["C"]) > 0.1          # why RANSAC: the fit over every pair is far off


def T44(pose):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = np.asarray(pose[:9]).reshape(3, 3), pose[9:]
    return torch.tensor(T)[None]


def test_chain_claim_on_the_restatement_and_the_oracle():
    """the claim of the GPU chain test, without a GPU: with half of the matches corrupted, ICP from the RANSAC pose reaches the truth and
    ICP from the fit over every match does not"""
    from oracle import dicp_oracle as O
    c = rr.chain_case(0)
    idx = c["corrupt"](c["gt"])
    out = rr.ransac_ref(c["x"], c["y"], idx, c["threshold"], hypotheses=256, seed=0, refine=1)
    keep = idx >= 0
    plain = rr.kabsch(c["x"][keep], c["y"][idx[keep]])[0]
    assert rr.rotation_error(out["pose"][:9], c["R"]) < 5e-3 and rr.rotation_error(plain[:9], c["R"]) > 0.5
    assert not out["inliers"][c["bad"]].any()
    xs, ys = torch.tensor(c["x"].astype(np.float64))[None], torch.tensor(c["y"].astype(np.float64))[None]
    err = {}
    for name, p in (("ransac", out["pose"]), ("plain", plain)):
        res = O.icp_batched(xs, ys, T44(p), torch.ones(1, 3 * xs.shape[1], dtype=torch.float64), icp_type="pt2pt", differentiable=False, max_iterations=20,
                            tolerance=1e-9)
        err[name] = rr.rotation_error(res["T"][0, :3, :3].numpy().reshape(-1), c["R"])
    assert err["ransac"] < 1e-2 and err["plain"] > 0.5, err


# ------------------------------------------------------------------ the Python fronts: ValueError before any device work
def _bad(fn, *args, **kw):
    with pytest.raises(ValueError):
        fn(*args, **kw)


def test_argument_checks_of_the_python_functions():
    x, y, idx = torch.zeros(5, 3), torch.zeros(7, 3), torch.zeros(5, dtype=torch.int64)
    for thr in (0, 0.0, -1.0, float("inf"), float("nan"), "0.1", None, True, torch.tensor(0.1)):
        _bad(ransac_correspondences, x, y, idx, thr)
    for H in (0, -1, 65537, 10.0, True, None):
        _bad(ransac_correspondences, x, y, idx, 0.1, hypotheses=H)
    for seed in (1.5, "1", True):
        _bad(ransac_correspondences, x, y, idx, 0.1, seed=seed)
    for R in (-1, 9, 1.0, True, None):
        _bad(ransac_correspondences, x, y, idx, 0.1, refine=R)
    _bad(ransac_correspondences, x, y, idx, 0.1, return_hypothesis=1)
    # the forms and checks of align_correspondences
    _bad(ransac_correspondences, x, y, idx.float(), 0.1)
    _bad(ransac_correspondences, x, y, idx[:4], 0.1)
    _bad(ransac_correspondences, x, y, idx + 7, 0.1)
    _bad(ransac_correspondences, x, y, idx, 0.1, weight=torch.ones(5, dtype=torch.float64))
    _bad(ransac_correspondences, x, y, idx, 0.1, weight=torch.ones(4))
    _bad(ransac_correspondences, x[:, :2], y, idx, 0.1)
    _bad(ransac_correspondences, [x], [y], idx, 0.1)
    _bad(ransac_correspondences, x, y, idx, 0.1, x_rows=torch.tensor([3]))
    _bad(ransac_correspondences, x[None], y[None], idx[None], 0.1, x_rows=torch.tensor([6]))
    _bad(ransac_correspondences, x.half(), y.half(), idx, 0.1)
    T = torch.eye(4)
    _bad(correspondence_residuals, x, y, idx, T.double())
    _bad(correspondence_residuals, x, y, idx, T[None])
    _bad(correspondence_residuals, x, y, idx, T[:3])
    _bad(correspondence_residuals, x, y, idx, None)
    _bad(correspondence_residuals, x[None], y[None], idx[None], T)
    _bad(correspondence_residuals, x[None], y[None], idx[None], T[None].repeat(2, 1, 1))
    _bad(correspondence_residuals, x, y, idx + 7, T)
    _bad(correspondence_residuals, x, y, idx.float(), T)
    _bad(correspondence_residuals, x, y, idx, T, x_rows=torch.tensor([3]))
