"""ransac_correspondences / correspondence_residuals on the MI355X (dicp_amd/register.py; csrc/ransac.hip), against the numpy restatement
tests/ransac_ref.py.

1  every stage on ragged batches of three clouds, float32 and float64, pad rows holding NaN and 1e30: the packed pairs, P, the samples
   integer for integer; counts, best, best_count, I_0 .. I_R and inliers bit for bit, the reference evaluated on the kernel's own stored
   poses; the stored poses against float64 Kabsch inside the bound of tests/ransac_cases.py;
2  shapes at the edges of the score kernel's tiles: P in {0, 1, 2, 3, 4, S - 1, S, S + 1, 2 S + 1} (S = dicp_ransac_slice()) and
   H in {1, 63, 64, 65, 255, 256, 257, 1000};
3  designed inputs through _poses: a tie, a pair on the threshold and one step above it, NaN and inf poses, all pairs inliers of every
   pose, idx >= m on a device tensor, duplicate points in a sample;
4  end to end: the counts against correspondence_residuals, reproducibility, the final fit and its gradients against
   align_correspondences on the returned mask, the recovery case, the chain descriptors -> match_features -> ransac -> ICP with half of
   the matches corrupted;  5  a call with an int seed in a captured graph.
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import _lib
from dicp_amd import match as M
from dicp_amd.ICP import ICP
from dicp_amd.match import align_correspondences, correspondence_residuals, match_features, ransac_correspondences

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_cases as rc  # noqa: E402
import ransac_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

TD = {np.float32: torch.float32, np.float64: torch.float64}
DTYPES = [np.float32, np.float64]
H_CASES = (1, 63, 64, 65, 255, 256, 257, 1000)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and (torch.equal(bits(a), bits(b)) if a.dtype.is_floating_point else torch.equal(a, b))


@pytest.fixture(scope="module")
def S():
    return _lib.load().dicp_ransac_slice()


def stages(x, y, idx, thr, H, seed, refine, weight=None, x_rows=None, poses=None):
    """_ransac_stages on numpy inputs (batches)"""
    rows = None if x_rows is None else torch.tensor(x_rows, dtype=torch.int32).cuda()
    _, _, xd, yd, idx_d, w, rows_d = M._pair_arguments(dev(x), dev(y), dev(idx), None if weight is None else dev(weight), rows, "test")
    return M._ransac_stages(xd, yd, idx_d, w, rows_d, thr, H, seed, refine, _poses=None if poses is None else dev(poses))


def cloud(rng, n, m, P, dtype, rows=None, inlier_ratio=0.6, noise=0.01):
    """One cloud with exactly P live pairs among its first `rows` rows: x in a unit cube around (1, 1, 1), y = C x + r + noise for the
    inliers and uniform for the rest, idx an injection into y.  The other rows are not live, each for another reason in turn: idx < 0, a
    NaN in x, an inf in the matched row of y; rows at and past `rows` are padding holding NaN and 1e30.  Some live rows name a row of y at or
    past m (clamped to m - 1).  -> x (n, 3), y (m, 3), idx (n,) int64"""
    rows = n if rows is None else rows
    C, r = rr.rotation(rng), rng.uniform(-0.5, 0.5, 3)
    x = rng.uniform(0.5, 1.5, (n, 3))
    to = rng.permutation(m - 1)[:n] if n <= m - 1 else rng.integers(0, m - 1, n)
    y = rng.uniform(-1.0, 3.0, (m, 3))
    good = rng.random(n) < inlier_ratio
    y[to[good]] = x[good] @ C.T + r + noise * rng.standard_normal((int(good.sum()), 3))
    idx = to.astype(np.int64)
    livepos = np.sort(rng.permutation(rows)[:P])
    dead = np.setdiff1d(np.arange(rows), livepos)
    x, y = x.astype(dtype), y.astype(dtype)
    for k, i in enumerate(dead):
        if k % 3 == 0:
            idx[i] = -1 - (k % 5)
        elif k % 3 == 1:
            x[i, k % 2] = np.nan
        elif n <= m - 1:
            y[idx[i], 2] = np.inf
        else:
            idx[i] = -1
    if P > 8:                                                   # a clamped index: the last row of y, matched to x's inlier motion
        i = livepos[3]
        y[m - 1] = (x[i].astype(np.float64) @ C.T + r).astype(dtype)
        idx[i] = m + 5
    x[rows:] = np.nan
    x[rows + 1::2] = 1e30
    idx[rows:] = rng.integers(0, m, n - rows)
    return x, y, idx


def check_stages(st, x, y, idx, thr, H, seed, refine, x_rows, expect_share=True):
    """every stage of every cloud against the restatement evaluated on the kernel's own poses"""
    N = x.shape[0]
    dtype = x.dtype.type
    for b in range(N):
        rows_b = None if x_rows is None else x_rows[b]
        poses = host(st["poses"][b])
        ref = rr.ransac_ref(x[b], y[b], idx[b], thr, H, seed, refine, x_rows=rows_b, cloud=b, poses=poses, round_poses=[host(p[b]) for p in st["round_poses"]])
        P = ref["P"]
        assert int(st["P"][b]) == P, b
        assert np.array_equal(host(st["live"][b]), rr.live_mask(x[b], y[b], idx[b], rows_b))
        assert rc.same_bits(host(st["pairs"][b, :P]), ref["pairs"]) and np.array_equal(host(st["index"][b, :P]), ref["rows"])
        assert np.array_equal(host(st["samples"][b]), ref["samples"]), b
        assert np.array_equal(host(st["counts"][b]), ref["counts"]), b
        assert int(st["best"][b]) == ref["best"] and int(st["best_count"][b]) == ref["best_count"], b
        assert rc.same_bits(host(st["pose_best"][b]), ref["pose_best"])
        for j, (got, want) in enumerate(zip(st["sets"], ref["sets"])):
            assert np.array_equal(host(got[b]), want), (b, j)
        assert np.array_equal(host(st["inliers"][b]), ref["inliers"])
        if P >= 3:
            ok, share, wc, wr = rc.poses_hold(poses, ref["pairs"], ref["samples"])
            print("cloud %d %s P %d H %d: share %.3f, worst dC / bound %.3g, worst dr / bound %.3g" % (b, np.dtype(dtype).name, P, H, share, wc, wr))
            if share > 0:
                assert ok, (b, wc, wr)
            if expect_share and P >= 100 and H >= 200:
                assert share >= rc.MIN_SHARE
        else:
            assert np.array_equal(poses, np.tile(rr.IDENTITY.astype(dtype), (H, 1)))


def batch(rng, dtype, n, m, Ps, rows):
    cs = [cloud(rng, n, m, P, dtype, rows=r) for P, r in zip(Ps, rows)]
    return tuple(np.stack([c[k] for c in cs]) for k in range(3))


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("refine", (0, 2))
def test_stages_on_ragged_batches(dtype, refine):
    rng = np.random.default_rng(3 + refine)
    rows = [400, 371, 290]
    x, y, idx = batch(rng, dtype, 400, 450, (330, 250, 120), rows)
    w = rng.uniform(0.5, 1.5, (3, 400)).astype(dtype)
    for weight in (None, w):
        st = stages(x, y, idx, 0.04, 300, 12345, refine, weight=weight, x_rows=rows)
        check_stages(st, x, y, idx, 0.04, 300, 12345, refine, rows)
        assert len(st["sets"]) == refine + 1 and len(st["accepted"]) == refine
        for b in range(3):
            assert int(st["best_count"][b]) > 0.4 * int(st["P"][b])        # the motion is found
            assert int(st["sets"][0][b].sum()) == int(st["best_count"][b])


# ------------------------------------------------------------------ 2
def edge_groups(S):
    return ((0, 3, S - 1), (1, 4, S), (2, S + 1, 2 * S + 1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", H_CASES)
def test_tile_edges_over_H(S, dtype, H):
    Ps = edge_groups(S)[H % 3]
    n = 2 * S + 40
    rng = np.random.default_rng(H)
    x, y, idx = batch(rng, dtype, n, n + 30, Ps, (n, n - 7, n))
    st = stages(x, y, idx, 0.04, H, 77, 1, x_rows=[n, n - 7, n])
    check_stages(st, x, y, idx, 0.04, H, 77, 1, [n, n - 7, n])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("group", (0, 1, 2))
def test_tile_edges_over_P(S, dtype, group):
    Ps = edge_groups(S)[group]
    n = min(4 * S + 70, 1100)
    rng = np.random.default_rng(group)
    x, y, idx = batch(rng, dtype, n, 900, Ps, (n, n, n - 1))       # n > m - 1: several rows of x share a row of y
    st = stages(x, y, idx, 0.04, 257, 5, 1, x_rows=None if group == 0 else [n, n, n - 1])
    check_stages(st, x, y, idx, 0.04, 257, 5, 1, None if group == 0 else [n, n, n - 1])
    for b, P in enumerate(Ps):
        if P < 3:
            T, inl, best, bc, Tb = ransac_correspondences(dev(x[b]), dev(y[b]), dev(idx[b]), 0.04, hypotheses=8, seed=1, return_hypothesis=True)
            assert int(best[0]) == -1 and int(bc[0]) == 0 and not inl.any() and torch.equal(Tb[0], torch.eye(4, dtype=TD[dtype]).cuda())
            assert same(T, align_correspondences(dev(x[b]), dev(y[b]), torch.full((n,), -1, dtype=torch.int64).cuda()))


# ------------------------------------------------------------------ 3
IDENT = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_designed_poses(S, dtype):
    rng = np.random.default_rng(9)
    n, H = 2 * S + 3, 70
    x = rng.uniform(-1, 1, (n, 3)).astype(dtype)
    y = x.copy()
    k = n // 2 + 2
    y[:k] += dtype(1.0)                                         # k pairs fit the shift by (1, 1, 1) exactly, the other n - k < k the identity
    idx = np.arange(n, dtype=np.int64)
    shift = np.array(IDENT[:9] + [1, 1, 1], dtype=dtype)
    poses = np.full((1, H, 12), np.nan, dtype=dtype)            # a NaN pose scores 0
    poses[0, 5], poses[0, 2] = shift, shift                     # the same pose twice: the lower h wins
    poses[0, 7] = np.array(IDENT, dtype=dtype)
    poses[0, 8] = np.array(IDENT[:9] + [np.inf, 0, 0], dtype=dtype)     # an inf pose scores 0
    poses[0, 9] = np.array([np.inf] + IDENT[1:], dtype=dtype)
    st = stages(x[None], y[None], idx[None], 1e-3, H, 0, 0, poses=poses)
    counts = host(st["counts"][0])
    assert counts[5] == k and counts[2] == k and counts[7] == n - k
    assert int(st["best"][0]) == 2 and int(st["best_count"][0]) == k
    assert counts[8] == 0 and counts[9] == 0 and counts[0] == 0 and counts.sum() == 2 * k + (n - k)
    assert np.array_equal(host(st["samples"]), np.full((1, H, 3), -1))
    assert np.array_equal(host(st["inliers"][0]), np.arange(n) < k)
    ref = rr.score(poses[0], np.concatenate((x, y), axis=1), 1e-3)
    assert np.array_equal(counts, ref[0]) and ref[1] == 2
    # all pairs inliers of every pose: best is 0
    st = stages(x[None], x[None], idx[None], 0.5, H, 0, 0, poses=np.tile(np.array(IDENT, dtype=dtype), (1, H, 1)))
    assert int(st["best"][0]) == 0 and int(st["best_count"][0]) == n and np.all(host(st["counts"]) == n) and bool(st["inliers"].all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_on_the_threshold_and_one_step_above(dtype):
    T = dtype
    e_on = T(0.25)
    e_out = np.nextafter(e_on, T(1))
    x = np.zeros((1, 6, 3), dtype=T)
    y = np.zeros((1, 6, 3), dtype=T)
    y[0, 0, 0] = -e_on                                          # d = 0.0625 = thr2 exactly: in
    y[0, 1, 1] = e_out                                          # one step above: out
    y[0, 2, 2] = e_on
    y[0, 3] = (e_on, e_out, 0)                                  # far out
    idx = np.arange(6, dtype=np.int64)[None]
    poses = np.array(IDENT, dtype=T)[None, None]
    st = stages(x, y, idx, 0.25, 1, 0, 0, poses=poses)
    assert list(host(st["inliers"][0])) == [True, False, True, False, True, True]
    assert int(st["counts"][0, 0]) == 4 and int(st["best_count"][0]) == 4
    d2 = correspondence_residuals(dev(x), dev(y), dev(idx), torch.eye(4, dtype=TD[T]).cuda()[None])
    assert d2.dtype == TD[T] and not d2.requires_grad
    assert float(d2[0, 0]) == 0.0625 and float(d2[0, 1]) > 0.0625 and float(d2[0, 4]) == 0.0
    assert rc.same_bits(host(d2[0]), rr.residuals_rows(np.array(IDENT, dtype=T), x[0], y[0], idx[0]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_clamped_index_and_rows_that_are_not_live(dtype):
    rng = np.random.default_rng(4)
    n, m = 40, 9
    x = rng.standard_normal((2, n, 3)).astype(dtype)
    y = rng.standard_normal((2, m, 3)).astype(dtype)
    idx = rng.integers(-2, m + 6, (2, n)).astype(np.int64)      # negative, in range, and at or past m (clamped to m - 1)
    x[0, 5, 1] = np.nan
    y[1, 3, 0] = np.inf
    pose = rng.standard_normal((2, 12)).astype(dtype)
    T = np.zeros((2, 4, 4), dtype=dtype)
    T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = pose[:, :9].reshape(2, 3, 3), pose[:, 9:], 1
    for idx_t in (dev(idx), dev(idx.astype(np.int32))):
        d2 = correspondence_residuals(dev(x), dev(y), idx_t, dev(T), x_rows=torch.tensor([n, 31]).cuda())
        for b, rows in enumerate((n, 31)):
            want = rr.residuals_rows(pose[b], x[b], y[b], idx[b], rows)
            assert rc.same_bits(host(d2[b]), want)
            assert np.isinf(want[idx[b] < 0]).all() and np.isfinite(want[(idx[b] >= m) & (np.arange(n) < rows) & np.isfinite(x[b]).all(1)]).all()
    single = correspondence_residuals(dev(x[0]), dev(y[0]), dev(idx[0]), dev(T[0]))
    assert rc.same_bits(host(single), rr.residuals_rows(pose[0], x[0], y[0], idx[0]))
    on_cpu = correspondence_residuals(torch.from_numpy(x[0]), torch.from_numpy(y[0]), torch.from_numpy(np.clip(idx[0], -2, m - 1)), torch.from_numpy(T[0]))
    assert not on_cpu.is_cuda and rc.same_bits(on_cpu.numpy(), rr.residuals_rows(pose[0], x[0], y[0], np.clip(idx[0], -2, m - 1)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicate_points_in_a_sample(dtype):
    rng = np.random.default_rng(6)
    pairs = rc.cube_pairs(rng, 4, dtype)
    x, y = pairs[:, :3].copy(), pairs[:, 3:].copy()
    x[1], y[1] = x[0], y[0]
    x[2], y[2] = x[0], y[0]                                     # three of the four pairs are one point: most samples are rank-deficient
    idx = np.arange(4, dtype=np.int64)
    st = stages(x[None], y[None], idx[None], 0.01, 64, 3, 1)
    poses = host(st["poses"][0]).astype(np.float64)
    assert np.isfinite(poses).all() and np.allclose(np.linalg.det(poses[:, :9].reshape(-1, 3, 3)), 1.0, atol=1e-5)
    check_stages(st, x[None], y[None], idx[None], 0.01, 64, 3, 1, None, expect_share=False)
    assert int(st["best_count"][0]) >= 3


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("dtype", DTYPES)
def test_end_to_end_properties(dtype):
    rng = np.random.default_rng(21)
    rows = [350, 300, 350]
    x, y, idx = batch(rng, dtype, 350, 400, (300, 200, 5), rows)
    xd, yd, id_, rw = dev(x), dev(y), dev(idx), torch.tensor(rows).cuda()
    thr = 0.04
    thr2 = torch.full((), thr * thr, dtype=TD[dtype]).cuda()
    T0, in0, best, bc, Tb = ransac_correspondences(xd, yd, id_, thr, hypotheses=200, seed=5, refine=0, x_rows=rw, return_hypothesis=True)
    assert T0.shape == (3, 4, 4) and in0.shape == (3, 350) and in0.dtype == torch.bool and best.dtype == torch.int32 and bc.dtype == torch.int32
    d2 = correspondence_residuals(xd, yd, id_, Tb, x_rows=rw)
    assert torch.equal(in0, d2 <= thr2) and torch.equal(bc.long(), in0.sum(dim=1))
    T1, in1, best1, bc1, Tb1 = ransac_correspondences(xd, yd, id_, thr, hypotheses=200, seed=5, refine=2, x_rows=rw, return_hypothesis=True)
    assert torch.equal(best, best1) and torch.equal(bc, bc1) and same(Tb, Tb1)
    assert bool((bc1.long() <= in1.sum(dim=1)).all())
    again = ransac_correspondences(xd, yd, id_, thr, hypotheses=200, seed=5, refine=2, x_rows=rw, return_hypothesis=True)
    for a, b in zip((T1, in1, best1, bc1, Tb1), again):
        assert same(a, b)
    s5 = stages(x, y, idx, thr, 200, 5, 0, x_rows=rows)["samples"]
    s6 = stages(x, y, idx, thr, 200, 6, 0, x_rows=rows)["samples"]
    s5w = stages(x, y, idx, thr, 200, 5 + (1 << 32), 0, x_rows=rows)["samples"]
    assert not torch.equal(s5[:2], s6[:2]) and torch.equal(s5, s5w)
    a = ransac_correspondences(xd, yd, id_, thr, hypotheses=64, seed=None, x_rows=rw)       # a drawn seed: torch's CPU generator decides
    torch.manual_seed(3)
    b = ransac_correspondences(xd, yd, id_, thr, hypotheses=64, seed=None, x_rows=rw, return_hypothesis=True)
    torch.manual_seed(3)
    c = ransac_correspondences(xd, yd, id_, thr, hypotheses=64, seed=None, x_rows=rw, return_hypothesis=True)
    assert a[0].shape == (3, 4, 4) and all(same(u, v) for u, v in zip(b, c))
    # single clouds and CPU tensors
    Ts, ins = ransac_correspondences(xd[0], yd[0], id_[0], thr, hypotheses=200, seed=5, refine=2)
    assert Ts.shape == (4, 4) and ins.shape == (350,) and same(Ts, T1[0]) and torch.equal(ins, in1[0])
    Tc, inc = ransac_correspondences(torch.from_numpy(x[0]), torch.from_numpy(y[0]), torch.from_numpy(np.minimum(idx[0], 399)), thr, hypotheses=200, seed=5, refine=2)
    assert not Tc.is_cuda and not inc.is_cuda and same(Tc.cuda(), T1[0]) and torch.equal(inc.cuda(), in1[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_final_fit_and_gradients_are_align_correspondences(dtype):
    rng = np.random.default_rng(22)
    x, y, idx = batch(rng, dtype, 300, 320, (300, 300, 300), [300, 300, 300])
    idx[1, ::3] = -1                                            # rows without a match; all values finite: the gradients are meaningful
    idx[2, 2:] = -1                                             # P = 2: no hypotheses
    w = rng.uniform(0.5, 1.5, (3, 300)).astype(dtype)
    g = dev(rng.standard_normal((3, 4, 4)).astype(dtype))
    leaves = [[dev(t).requires_grad_(True) for t in (x, y, w)] for _ in range(2)]
    T, inl = ransac_correspondences(leaves[0][0], leaves[0][1], dev(idx), 0.04, hypotheses=128, seed=1, refine=1, weight=leaves[0][2])
    assert T.requires_grad and not inl.requires_grad
    Ta = align_correspondences(leaves[1][0], leaves[1][1], torch.where(inl, dev(idx), torch.full_like(dev(idx), -1)), weight=leaves[1][2])
    assert same(T[:2].detach(), Ta[:2].detach())
    assert torch.equal(torch.isnan(T[2]), torch.isnan(Ta[2]))  # (P = 2: no hypotheses, align_correspondences' pose for no pairs at all)
    ga = torch.autograd.grad(T[:2], leaves[0], g[:2])
    gb = torch.autograd.grad(Ta[:2], leaves[1], g[:2])
    for u, v in zip(ga[::2], gb[::2]):                          # x and weight: stored once; y: float atomics in dicp_kabsch_bwd
        assert same(u[:2], v[:2])
    assert torch.allclose(ga[1][:2], gb[1][:2], rtol=1e-4 if dtype == np.float32 else 1e-10, atol=1e-5 if dtype == np.float32 else 1e-12)
    assert all(torch.isfinite(t[:2]).all() for t in ga)
    outliers = dev(rr.live_mask(x[0], y[0], idx[0])) & ~inl[0]
    assert (ga[0][0] != 0).any() and outliers.any() and not (ga[0][0][outliers] != 0).any()       # only the inliers are reached


@pytest.mark.parametrize("seed", range(5))
def test_recovery_case(seed):
    a = rr.recovery_case(seed)
    T, inl = ransac_correspondences(dev(a["x"]), dev(a["y"]), dev(a["idx"]), 0.05, hypotheses=256, seed=seed, refine=1)
    assert bool(inl[dev(a["truth"])].all())
    err = rr.rotation_error(host(T[:3, :3]).reshape(-1), a["C"])
    print("seed %d: inliers %d of %d true, rotation error %.3g" % (seed, int(inl.sum()), a["truth"].sum(), err))
    assert err < 5e-3


def test_full_chain_with_half_of_the_matches_corrupted():
    c = rr.chain_case(0)
    fx, fy, x, y = (dev(c[k]) for k in ("fx", "fy", "x", "y"))
    idx, _ = match_features(fx, fy, mutual=True, ratio=0.8)
    assert torch.equal(idx, dev(c["gt"]))
    idx = dev(c["corrupt"](host(idx)))
    T, inl = ransac_correspondences(x, y, idx, c["threshold"], hypotheses=256, seed=0, refine=1)
    assert not bool(inl[dev(c["bad"])].any())
    Tp = align_correspondences(x, y, idx)
    icp = ICP(icp_type="pt2pt", max_iterations=20, tolerance=1e-9)
    err = {}
    for name, T0 in (("ransac", T), ("plain", Tp)):
        out = icp.icp(x[None], y[None], T_init=T0[None])
        err[name] = rr.rotation_error(host(out["T"][0, :3, :3]).reshape(-1), c["R"])
    print("ICP from the RANSAC pose: %.3g rad; from the fit over every match: %.3g rad" % (err["ransac"], err["plain"]))
    assert err["ransac"] < 1e-2 and err["plain"] > 0.5


# ------------------------------------------------------------------ 5
def test_captured_call():
    def data(seed):
        rng = np.random.default_rng(seed)
        x, y, idx = batch(rng, np.float32, 300, 320, (250, 3, 140), [300, 300, 280])
        return {"x": dev(x), "y": dev(y), "idx": dev(idx), "rows": torch.tensor([300, 300, 280], dtype=torch.int32).cuda()}

    def run(s):
        return ransac_correspondences(s["x"], s["y"], s["idx"], 0.04, hypotheses=300, seed=42, refine=2, x_rows=s["rows"], return_hypothesis=True)
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
    for seed in (2, 3):
        fresh = data(seed)
        for key, t in fresh.items():
            static[key].copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(fresh)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(captured, eager)):
            assert same(a, b), (seed, i)
