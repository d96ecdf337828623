"""gnc_correspondences on the MI355X (dicp_amd/register.py; csrc/gnc.hip), against the g++ build of csrc/dicp_gnc.h (tests/gnc_cases.py).

1  the kernel against the g++ build, bit for bit -- weights, rounds, status, mu, T_last and the whole trace -- for P in {0, 1, 2, 3, 4}
   and one below / at / one above the wave (64) and the slot count (1024) of the sums' tree, and 2049; n = P and n = P + 70 with dead rows
   interleaved; both dtypes, both losses, with and without weight; a ragged batch of three clouds against its per-cloud calls;
2  the designed inputs of tests/test_gnc_host.py;
3  the returned T is align_correspondences on (where(weights > 0, idx, -1), weight weights) bit for bit, with its gradients;
   reproducibility; a call in a captured graph;
4  the recovery cases with the limits of tests/gnc_cases.py, the composition with prune_correspondences(order=2) for 60 true pairs of
   600, and the chain FPFH matches -> GNC -> ICP on the structured scene of tests/fpfh_cases.py.
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import match as M
from dicp_amd.fpfh import compute_fpfh
from dicp_amd.ICP import ICP
from dicp_amd.match import align_correspondences, gnc_correspondences, match_features, prune_correspondences, ransac_correspondences
from dicp_amd.normals import estimate_normals

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_cases as fc  # noqa: E402
import gnc_cases as gc  # noqa: E402
import gnc_ref as gr  # noqa: E402
import ransac_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

TD = {np.float32: torch.float32, np.float64: torch.float64}
DTYPES = gc.DTYPES
LOSSES = ("tls", "gm")
P_CASES = (0, 1, 2, 3, 4, 63, 64, 65, 1023, 1024, 1025, 2049)
same_bits = gc.same_bits


@pytest.fixture(scope="module")
def check():
    return gc.build()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and (torch.equal(bits(a), bits(b)) if a.dtype.is_floating_point else torch.equal(a, b))


def stages(x, y, idx, thr, loss, growth=1.4, iterations=128, weight=None, x_rows=None):
    """_gnc_stages with the trace on numpy inputs (batches)"""
    rows = None if x_rows is None else torch.tensor(x_rows, dtype=torch.int32).cuda()
    _, _, xd, yd, idx_d, w, rows_d = M._pair_arguments(dev(x), dev(y), dev(idx), None if weight is None else dev(weight), rows, "test")
    return M._gnc_stages(xd, yd, idx_d, w, rows_d, thr, loss, growth, iterations, trace=True)


def assert_is_the_host_build(check, st, x, y, idx, thr, loss, growth=1.4, iterations=128, weight=None, x_rows=None):
    """every output of every cloud of the batch, bit for bit; -> the g++ build's results"""
    out = []
    for b in range(x.shape[0]):
        h = gc.header_call(check, x[b], y[b], idx[b], thr, loss, growth, iterations, None if weight is None else weight[b], None if x_rows is None else x_rows[b])
        what = (b, loss, h["pairs"].shape[0], h["rounds"], h["status"])
        assert int(st["P"][b]) == h["pairs"].shape[0], what
        assert (int(st["rounds"][b]), int(st["status"][b])) == (h["rounds"], h["status"]), what
        assert same_bits(host(st["mu"][b]), np.float64(h["mu"])), what
        assert same_bits(host(st["trace"][b]), h["trace"]), what
        assert same_bits(host(st["pose_last"][b]), h["pose_last"]), what
        assert same_bits(host(st["weights"][b]), h["weights"]), what
        out.append(h)
    return out


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("P", P_CASES)
def test_kernel_is_the_host_build(check, dtype, loss, P):
    rng = np.random.default_rng(100 + P)
    for extra in (0, 70):
        if P + extra == 0:
            continue
        x, y, idx = gc.rows_cloud(rng, P, extra, dtype)
        w = rng.uniform(0.5, 1.5, x.shape[0]).astype(dtype)
        for weight in (None, w):
            wb = None if weight is None else weight[None]
            st = stages(x[None], y[None], idx[None], 0.04, loss, weight=wb)
            h = assert_is_the_host_build(check, st, x[None], y[None], idx[None], 0.04, loss, weight=wb)[0]
            assert h["status"] == (gr.TOO_FEW if P < 3 else h["status"]) and (P < 64 or h["rounds"] > 5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("loss", LOSSES)
def test_ragged_batch_against_its_per_cloud_calls(check, dtype, loss):
    rng = np.random.default_rng(11)
    n, m, rows, Ps = 1400, 1500, [1400, 371, 1290], (1100, 250, 2)
    xs, ys, ids = [], [], []
    for P, r in zip(Ps, rows):
        x, y, idx = gc.rows_cloud(rng, P, r - P, dtype, m_extra=m - r)
        pad = np.full((n - r, 3), np.nan, dtype)
        pad[1::2] = 1e30                                        # the rows past the count hold NaN and 1e30 and live-looking indices
        xs.append(np.concatenate((x, pad)))
        ys.append(y)
        ids.append(np.concatenate((idx, rng.integers(0, m, n - r))))
    x, y, idx = np.stack(xs), np.stack(ys), np.stack(ids)
    w = rng.uniform(0.5, 1.5, (3, n)).astype(dtype)
    for weight in (None, w):
        st = stages(x, y, idx, 0.04, loss, weight=weight, x_rows=rows)
        assert_is_the_host_build(check, st, x, y, idx, 0.04, loss, weight=weight, x_rows=rows)
        kw = dict(loss=loss, return_info=True)
        batch = gnc_correspondences(dev(x), dev(y), dev(idx), 0.04, weight=None if weight is None else dev(weight), x_rows=torch.tensor(rows).cuda(), **kw)
        assert batch[0].shape == (3, 4, 4) and batch[1].shape == (3, n) and batch[2].dtype == torch.int32 and batch[4].dtype == torch.float64
        for b, r in enumerate(rows):
            one = gnc_correspondences(dev(x[b, :r]), dev(y[b]), dev(idx[b, :r]), 0.04, weight=None if weight is None else dev(weight[b, :r]), **kw)
            assert one[0].shape == (4, 4) and one[1].shape == (r,)
            assert same(one[1], batch[1][b, :r]) and not bool(batch[1][b, r:].any())
            for k in (2, 3, 4, 5):
                assert same(one[k][0], batch[k][b]), (b, k)
            if Ps[b] >= 3:
                assert same(one[0], batch[0][b])
            else:
                assert torch.equal(torch.isnan(one[0]), torch.isnan(batch[0][b])) and int(one[3][0]) == gr.TOO_FEW


# ------------------------------------------------------------------ 2
def as_cloud(pairs):
    """packed pairs -> x (1, P, 3), y (1, P, 3), idx (1, P)"""
    return pairs[None, :, :3].copy(), pairs[None, :, 3:].copy(), np.arange(pairs.shape[0], dtype=np.int64)[None]


@pytest.mark.parametrize("dtype", DTYPES)
def test_designed_inputs(check, dtype):
    rng = np.random.default_rng(5)
    a, thr = gc.half_c2_case()
    x, y, idx = as_cloud(gc.flat_square(a, dtype))
    for t, loss in ((thr, "tls"), (float(np.nextafter(thr, 0.0)), "tls"), (thr, "gm")):
        h = assert_is_the_host_build(check, stages(x, y, idx, t, loss), x, y, idx, t, loss)[0]
        assert (h["rounds"] == 0) == (t == thr and loss == "tls")                                    # 2 dmax exactly c2 stops at once
    x, y, idx = as_cloud(rng.uniform(-1, 1, (6, 6)).astype(dtype))                                   # a round that trips the guard
    h = assert_is_the_host_build(check, stages(x, y, idx, 1e-3, "tls"), x, y, idx, 1e-3, "tls")[0]
    assert h["status"] == gr.GUARDED and h["rounds"] >= 1
    x, y, idx = as_cloud(gc.noisy_cloud(rng, 200, dtype))
    for loss in LOSSES:
        for it, g in ((1, 1.4), (7, 1.4), (256, 1.05), (128, 16.0)):                                 # the cap, the ends of growth
            h = assert_is_the_host_build(check, stages(x, y, idx, 0.04, loss, g, it), x, y, idx, 0.04, loss, g, it)[0]
            assert it >= 8 or (h["rounds"], h["status"]) == (it, gr.CAPPED)
    # user weights of 0, below 0 and NaN: rows that are not live
    x, y, idx = gc.rows_cloud(rng, 120, 30, dtype)
    w = rng.uniform(0.5, 1.5, 150).astype(dtype)
    off = rng.permutation(np.flatnonzero(rr.live_mask(x, y, idx)))[:9]
    w[off[:3]], w[off[3:6]], w[off[6:]] = 0.0, -1.0, np.nan
    for loss in LOSSES:
        st = stages(x[None], y[None], idx[None], 0.04, loss, weight=w[None])
        assert_is_the_host_build(check, st, x[None], y[None], idx[None], 0.04, loss, weight=w[None])
        assert int(st["P"][0]) == 111 and not bool(st["weights"][0][dev(off)].any())


def test_a_residual_that_is_not_finite(check):
    rng = np.random.default_rng(8)
    pairs = gc.noisy_cloud(rng, 60, np.float64, inlier_ratio=0.8)
    pairs[7, :3] = 1e200
    u = np.ones((1, 60))
    u[0, 7] = 1e-250
    x, y, idx = as_cloud(pairs)
    for loss in LOSSES:
        h = assert_is_the_host_build(check, stages(x, y, idx, 0.04, loss, weight=u), x, y, idx, 0.04, loss, weight=u)[0]
        assert h["status"] == gr.CONVERGED and h["weights"][7] == 0 and (h["weights"] > 0).sum() > 30
        h = assert_is_the_host_build(check, stages(x, y, idx, 0.04, loss), x, y, idx, 0.04, loss)[0]
        assert (h["rounds"], h["status"]) == (0, gr.CONVERGED if loss == "tls" else gr.GUARDED)


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("loss", LOSSES)
def test_final_fit_and_gradients_are_align_correspondences(dtype, loss):
    rng = np.random.default_rng(22)
    cs = [gc.rows_cloud(rng, 300, 0, dtype, m_extra=20) for _ in range(3)]
    x, y, idx = (np.stack([c[k] for c in cs]) for k in range(3))
    idx[1, ::3] = -1                                            # rows without a match; all values finite: the gradients are meaningful
    idx[2, 2:] = -1                                             # P = 2: nothing runs
    w = rng.uniform(0.5, 1.5, (3, 300)).astype(dtype)
    g = dev(rng.standard_normal((3, 4, 4)).astype(dtype))
    for with_weight in (True, False):
        leaves = [[dev(t).requires_grad_(True) for t in (x, y, w)] for _ in range(2)]
        T, wg = gnc_correspondences(leaves[0][0], leaves[0][1], dev(idx), 0.04, loss=loss, weight=leaves[0][2] if with_weight else None)
        assert T.requires_grad and not wg.requires_grad and wg.dtype == TD[dtype] and wg.shape == (3, 300)
        assert not bool(wg[2].any()) and not bool(wg[1, ::3].any()) and bool((wg[0] > 0).sum() >= 3)
        kept = torch.where(wg > 0, dev(idx), torch.full_like(dev(idx), -1))
        Ta = align_correspondences(leaves[1][0], leaves[1][1], kept, weight=leaves[1][2] * wg if with_weight else wg)
        assert same(T[:2].detach(), Ta[:2].detach()) and torch.equal(torch.isnan(T[2]), torch.isnan(Ta[2]))
        n_leaves = 3 if with_weight else 2
        ga = torch.autograd.grad(T[:2], leaves[0][:n_leaves], g[:2])
        gb = torch.autograd.grad(Ta[:2], leaves[1][:n_leaves], g[:2])
        for u, v in zip(ga[::2], gb[::2]):                      # x and weight: stored once; y: float atomics in dicp_kabsch_bwd
            assert same(u[:2], v[:2])
        assert torch.allclose(ga[1][:2], gb[1][:2], rtol=1e-4 if dtype == np.float32 else 1e-10, atol=1e-5 if dtype == np.float32 else 1e-12)
        assert all(torch.isfinite(t[:2]).all() for t in ga) and bool((ga[0][0] != 0).any())
        dropped = (dev(idx)[0] >= 0) & ~(wg[0] > 0)
        assert bool(dropped.any()) == (loss == "tls") and not bool((ga[0][0][dropped] != 0).any())    # only the pairs that kept weight are reached


@pytest.mark.parametrize("loss", LOSSES)
def test_three_calls_give_the_same_bytes(loss):
    rng = np.random.default_rng(31)
    cs = [gc.rows_cloud(rng, P, 2100 - P, np.float32, m_extra=20) for P in (2049, 1500, 700)]
    x, y, idx = (dev(np.stack([c[k] for c in cs])) for k in range(3))
    runs = [gnc_correspondences(x, y, idx, 0.04, loss=loss, return_info=True) for _ in range(3)]
    for other in runs[1:]:
        assert all(same(a, b) for a, b in zip(runs[0], other))
    xc, yc, ic = x.cpu(), y.cpu(), idx.cpu()
    on_cpu = gnc_correspondences(xc, yc, ic, 0.04, loss=loss, return_info=True)                     # CPU tensors: computed on the GPU, returned on the CPU
    assert not any(t.is_cuda for t in on_cpu) and all(same(a.cuda(), b) for a, b in zip(on_cpu, runs[0]))
    i32 = gnc_correspondences(x, y, idx.to(torch.int32), 0.04, loss=loss, return_info=True)
    assert all(same(a, b) for a, b in zip(i32, runs[0]))


def test_captured_call():
    def data(seed):
        rng = np.random.default_rng(seed)
        cs = [gc.rows_cloud(rng, P, 300 - P, np.float32, m_extra=20) for P in (250, 3, 140)]
        x, y, idx = (np.stack([c[k] for c in cs]) for k in range(3))
        return {"x": dev(x), "y": dev(y), "idx": dev(idx), "rows": torch.tensor([300, 300, 280], dtype=torch.int32).cuda()}

    def run(s):
        return gnc_correspondences(s["x"], s["y"], s["idx"], 0.04, loss="tls", x_rows=s["rows"], return_info=True)
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


# ------------------------------------------------------------------ 4
# The returned T is the closed form in the points' dtype over the pairs that kept weight; the limits of tests/gnc_cases.py are those of the
# kernel's own double pose.  float32 moments of coordinates up to s = 10 over a covariance whose second singular value is about 8 move a
# rotation by K_C 2^-24 s^2 / w_2 = 56 x 6e-8 x 12.5 = 4e-5 (the bound of tests/ransac_cases.py in float32): 1e-4 covers it.
T_SLACK = 1e-4


@pytest.mark.parametrize("case", gc.recovery_cases(), ids=lambda c: c[0] if isinstance(c, tuple) else None)
def test_recovery(case):
    name, a, thr, limit = case
    for loss in LOSSES:
        T, w, rounds, status, mu, T_last = gnc_correspondences(dev(a["x"]), dev(a["y"]), dev(a["idx"]), thr, loss=loss, return_info=True)
        err_last = rr.rotation_error(host(T_last[0, :3, :3]).reshape(-1), a["C"])
        err = rr.rotation_error(host(T[:3, :3]).reshape(-1), a["C"])
        print("%s %s: rounds %d status %d, rotation error of T_last %.3g and of T %.3g (limit %.3g)" % (name, loss, int(rounds[0]), int(status[0]), err_last, err, limit))
        assert err_last <= limit and err <= limit + T_SLACK and int(status[0]) == gr.CONVERGED
        if loss == "tls" and name.startswith("compat"):
            assert torch.equal(w > 0, dev(a["truth"])) and bool((w[dev(a["truth"])] == 1).all())


# "recovers" for 60 true pairs at noise 0.01 in a 10-unit cube: the noise-limited rotation error is about noise / (spread sqrt(60)) =
# 0.01 / (2.9 x 7.7) = 4.5e-4 rad per axis; the limit is ten times that, the 5e-3 rad of test_gpu_ransac.test_recovery_case.
COMPOSITION_LIMIT = 5e-3


@pytest.mark.parametrize("seed", range(5))
def test_composition_with_second_order_pruning(seed):
    a, thr, keep = gc.composition_case(seed)
    x, y, idx = dev(a["x"]), dev(a["y"]), dev(a["idx"])
    kept, _ = prune_correspondences(x, y, idx, thr, keep=keep, order=2)
    for loss in LOSSES:
        T, w, rounds, status, mu, T_last = gnc_correspondences(x, y, kept, thr, loss=loss, return_info=True)
        err = rr.rotation_error(host(T[:3, :3]).reshape(-1), a["C"])
        alone = rr.rotation_error(host(gnc_correspondences(x, y, idx, thr, loss=loss)[0][:3, :3]).reshape(-1), a["C"])
        print("seed %d %s: %d true pairs of %d kept; pruned then GNC %.3g rad (status %d), GNC alone %.3g rad"
              % (seed, loss, int((kept >= 0)[dev(a["truth"])].sum()), int((kept >= 0).sum()), err, int(status[0]), alone))
        assert err <= COMPOSITION_LIMIT


def test_full_chain_on_the_structured_scene():
    """The chain of test_gpu_fpfh.test_end_to_end_registration with gnc_correspondences in RANSAC's place: FPFH matches -> GNC -> ICP ends
    where the RANSAC chain ends, inside that test's limits against the truth and next to the RANSAC chain's own end."""
    P = fc.scene(0, 1500)
    mv = fc.moved_copy(P, seed=0, keep=0.85, angle=1.0, noise=0.002, axis=fc.E2E_AXIS)
    y, x = dev(P.astype(np.float32)), dev(mv["x"].astype(np.float32))
    vp_y = torch.tensor(fc.VIEWPOINT, dtype=torch.float32)
    vp_x = torch.tensor(fc.VIEWPOINT @ mv["R"].T + mv["t"], dtype=torch.float32)
    ny = estimate_normals(y, k=16, viewpoint=vp_y)
    nx = estimate_normals(x, k=16, viewpoint=vp_x)
    fx, fy = compute_fpfh(x, nx, 0.8, k=32), compute_fpfh(y, ny, 0.8, k=32)
    idx, _ = match_features(fx, fy, mutual=True)
    thr = 0.15
    C_true, r_true = mv["R"].T, -mv["R"].T @ mv["t"]
    starts = {"ransac": ransac_correspondences(x, y, idx, thr, hypotheses=4096, seed=7, refine=2)[0]}
    for loss in LOSSES:
        T0, w, rounds, status, mu, _ = gnc_correspondences(x, y, idx, thr, loss=loss, return_info=True)
        print("GNC %s: %d rounds, status %d, %d of %d matches keep weight" % (loss, int(rounds[0]), int(status[0]), int((w > 0).sum()), int((idx >= 0).sum())))
        starts[loss] = T0
    icp = ICP(icp_type="pt2pt", max_iterations=30, tolerance=1e-9)
    end = {}
    for name, Ti in starts.items():
        Th = host(icp.icp(x[None], y[None], T_init=Ti[None])["T"][0]).astype(np.float64)
        end[name] = Th
        err = (rr.rotation_error(Th[:3, :3].reshape(-1), C_true), float(np.linalg.norm(Th[:3, 3] - r_true)))
        print("ICP from the %s pose: %.3g rad, %.3g m" % ((name,) + err))
        assert err[0] < 1e-2 and err[1] < 5e-2
    for loss in LOSSES:
        assert rr.rotation_error(end[loss][:3, :3].reshape(-1), end["ransac"][:3, :3].reshape(-1)) < 1e-3
        assert np.linalg.norm(end[loss][:3, 3] - end["ransac"][:3, 3]) < 1e-2
