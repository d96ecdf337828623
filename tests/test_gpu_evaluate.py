"""dicp_amd.evaluate on the MI355X (csrc/evaluate.hip), against the numpy restatement tests/evaluate_ref.py.

1  the kernels against the restatement, bit for bit, in both dtypes -- idx, d2, counts, the ten sums, fitness, rmse -- for a padded batch
   of three clouds with different row counts (one of them 0), n in {65, 257, 1000}, m = 700, H in {1, 5}, and the designed inputs of
   tests/evaluate_cases.py;
2  idx and d2 are ball_query(q, target, max_distance, k=1) bit for bit, q the restatement's transformed source, and counts their number;
3  three runs give the same bytes; poses evaluated together equal one call per pose;
4  the scene of tests/fpfh_cases.py: the true pose wins, fitness exactly 1, the rmse inside the derived bound of tests/evaluate_cases.py;
5  the pipeline ransac / gnc -> best_pose -> ICP -> evaluate_registration;
6  CPU tensors, the single-pair forms, the information matrix, a call in a captured graph.
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import evaluate as E
from dicp_amd.ball import ball_query
from dicp_amd.evaluate import best_pose, evaluate_registration, information_matrix
from dicp_amd.ICP import ICP
from dicp_amd.match import gnc_correspondences, ransac_correspondences

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaluate_cases as ec  # noqa: E402
import evaluate_ref as er  # noqa: E402
import ransac_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = ec.DTYPES
M = 700
same_bits = ec.same_bits
_BATCHES = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and (torch.equal(bits(a), bits(b)) if a.dtype.is_floating_point else torch.equal(a, b))


def batch(n, H, dtype):
    """Three padded clouds of very different magnitudes, NaN past the row counts, and the restatement of every cloud, computed once
    -> dict x (3, n, 3), y (3, M, 3), T (3, H, 4, 4), radius, srows, trows, ref [per cloud]"""
    key = (n, H, dtype)
    if key not in _BATCHES:
        srows, trows = [n, max(n - 30, 1), 0], [M, M - 60, M]
        xs, ys, Ts = [], [], []
        for b in range(3):
            x, y, T, radius = ec.magnitudes_case(100 * n + 10 * H + b, n, trows[b], H, dtype)
            x, y = x.copy(), np.concatenate((y, np.full((M - trows[b], 3), np.nan, dtype)))
            x[srows[b]:] = np.nan
            xs.append(x), ys.append(y), Ts.append(T)
        x, y, T = np.stack(xs), np.stack(ys), np.stack(Ts)
        ref = [er.evaluate_ref(x[b], y[b], T[b], radius, srows[b], trows[b]) for b in range(3)]
        _BATCHES[key] = dict(x=x, y=y, T=T, radius=radius, srows=srows, trows=trows, ref=ref)
    return _BATCHES[key]


def run_all(x, y, T, radius, srows=None, trows=None):
    """every output of the kernels for device tensors -> dict of numpy arrays with a leading (N, H)"""
    on_cpu, n, lead, sums, counts, fitness, rmse, idx, d2 = E._evaluate(x, y, T, radius, srows, trows, True, "test")
    return dict(idx=host(idx[:, :, :n]), d2=host(d2[:, :, :n]), counts=host(counts), sums=host(sums), fitness=host(fitness), rmse=host(rmse))


# ------------------------------------------------------------------ 1: bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", (1, 5))
@pytest.mark.parametrize("n", (65, 257, 1000))
def test_kernels_are_the_restatement(dtype, n, H):
    c = batch(n, H, dtype)
    srows, trows = (torch.tensor(c[k], dtype=torch.int32).cuda() for k in ("srows", "trows"))
    got = run_all(dev(c["x"]), dev(c["y"]), dev(c["T"]), c["radius"], srows, trows)
    for b in range(3):
        assert ec.differences({k: v[b] for k, v in got.items()}, c["ref"][b]) == [], b
    assert got["counts"][0, 0] >= 0.9 * n and (got["counts"][2] == 0).all() and (got["fitness"][2] == 0).all() and (got["rmse"][2] == 0).all()
    fit, rmse, counts, idx, d2 = evaluate_registration(dev(c["x"]), dev(c["y"]), dev(c["T"]), c["radius"], srows, trows, return_correspondences=True)
    assert fit.shape == rmse.shape == counts.shape == (3, H) and idx.shape == d2.shape == (3, H, n)
    assert (fit.dtype, rmse.dtype, counts.dtype, idx.dtype, d2.dtype) == (torch.float64, torch.float64, torch.int32, torch.int64, dev(c["x"]).dtype)
    assert not any(t.requires_grad for t in (fit, rmse, counts, idx, d2))
    for name, t in (("fitness", fit), ("rmse", rmse), ("counts", counts), ("idx", idx), ("d2", d2)):
        assert same_bits(host(t), got[name]), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(ec.designed(np.float32)))
def test_designed_inputs(dtype, name):
    case = ec.designed(dtype)[name]
    ref = ec.ref_of(case)
    rows = [None if case.get(k) is None else torch.tensor([case[k]], dtype=torch.int32).cuda() for k in ("x_rows", "y_rows")]
    got = run_all(dev(case["x"])[None], dev(case["y"])[None], dev(case["T"])[None], case["radius"], *rows)
    one = {k: v[0] for k, v in got.items()}
    assert ec.differences(one, ref) == []
    case["expect"](one)


# ------------------------------------------------------------------ 2: agreement with ball_query
@pytest.mark.parametrize("dtype", DTYPES)
def test_matches_are_ball_query_at_k_1(dtype):
    c = batch(257, 5, dtype)
    x, y, T = dev(c["x"]), dev(c["y"]), dev(c["T"])
    srows, trows = (torch.tensor(c[k], dtype=torch.int32).cuda() for k in ("srows", "trows"))
    _, _, counts, idx, d2 = evaluate_registration(x, y, T, c["radius"], srows, trows, return_correspondences=True)
    for h in range(5):
        q = dev(np.stack([c["ref"][b]["q"][h] for b in range(3)]))
        bd2, bidx = ball_query(q, y, c["radius"], k=1, x_rows=srows, y_rows=trows)
        assert same(bidx[..., 0], idx[:, h]) and same(bd2[..., 0], d2[:, h]), h
    assert torch.equal(counts.to(torch.int64), (idx >= 0).sum(-1))


# ------------------------------------------------------------------ 3: reproducibility, pose independence
@pytest.mark.parametrize("dtype", DTYPES)
def test_reproducible_and_independent_of_the_other_poses(dtype):
    c = batch(1000, 5, dtype)
    x, y, T = dev(c["x"]), dev(c["y"]), dev(c["T"])
    srows, trows = (torch.tensor(c[k], dtype=torch.int32).cuda() for k in ("srows", "trows"))
    runs = [run_all(x, y, T, c["radius"], srows, trows) for _ in range(3)]
    for other in runs[1:]:
        assert ec.differences(other, runs[0]) == []
    infos = [information_matrix(x, y, T, c["radius"], srows, trows) for _ in range(2)]
    assert same(infos[0], infos[1])
    for h in (0, 2, 4):
        alone = run_all(x, y, T[:, h:h + 1].contiguous(), c["radius"], srows, trows)
        assert ec.differences(alone, {k: v[:, h:h + 1] for k, v in runs[0].items()}) == [], h
        flat = run_all(x, y, T[:, h].contiguous(), c["radius"], srows, trows)                         # (N, 4, 4): the same call
        assert ec.differences(flat, alone) == []


# ------------------------------------------------------------------ 4: the scene
@pytest.mark.parametrize("dtype", DTYPES)
def test_scene(dtype):
    x, y, T = ec.scene_case(dtype)
    fit, rmse, counts = evaluate_registration(dev(x), dev(y), dev(T), ec.SCENE_DISTANCE)
    assert fit.shape == (3,)
    best, T_best = best_pose(dev(T), counts, rmse)
    print("scene %s: fitness %s rmse %s counts %s" % (np.dtype(dtype).name, host(fit), host(rmse), host(counts)))
    assert int(best) == 0 and same(T_best, dev(T)[0])
    assert float(fit[0]) == 1.0 and float(fit[1]) < 0.5 and float(fit[2]) < 0.5
    ref_fit, ref_rmse, ref_count = ec.brute_force64(x, y, T[0], ec.SCENE_DISTANCE)
    bound = ec.rmse_bound(x, T[0], ec.SCENE_DISTANCE, dtype)
    print("  rmse of the true pose %.12g, float64 numpy %.12g, bound %.3g" % (float(rmse[0]), ref_rmse, bound))
    assert int(counts[0]) == ref_count == 1275 and abs(float(rmse[0]) - ref_rmse) <= bound
    assert abs(ref_rmse - ec.SCENE_RMSE[0]) < 1e-2 * ec.SCENE_RMSE[0]


# ------------------------------------------------------------------ 5: the pipeline
def test_pipeline_ranks_candidates_and_checks_the_refinement():
    """ransac_ref.recovery_case(0): 300 rows, 120 of them with a counterpart at noise 0.005, the others' counterparts replaced by uniform
    rows.  max_distance = 0.05 is ten times the noise; ICP is given the same distance as its trim_dist, as a pipeline would (60 % of the
    rows have nothing to converge to).  Measured on an MI355X: both candidates at fitness 0.41 and rmse 0.00975; after ICP 0.41 and 0.0106."""
    a = rr.recovery_case(0)
    x, y, idx = dev(a["x"]), dev(a["y"]), dev(a["idx"])
    dist = 0.05
    T_ransac = ransac_correspondences(x, y, idx, 0.02, hypotheses=1024, seed=3)[0]
    T_gnc = gnc_correspondences(x, y, idx, 0.02)[0]
    cands = torch.stack((T_ransac, T_gnc))                                   # (2, 4, 4): the single-pair form
    fit, rmse, cnt = evaluate_registration(x, y, cands, dist)
    best, T0 = best_pose(cands, cnt, rmse)
    assert T0.shape == (4, 4) and same(T0, cands[int(best)])
    out = ICP(icp_type="pt2pt", max_iterations=30, tolerance=1e-9).icp(x[None], y[None], T_init=T0[None], trim_dist=dist)
    fit1, rmse1, cnt1 = evaluate_registration(x, y, out["T"][0].detach(), dist)
    print("pipeline: candidates fitness %s rmse %s, best %d; after ICP fitness %.6g rmse %.6g" % (host(fit), host(rmse), int(best), float(fit1), float(rmse1)))
    assert float(fit1) >= float(fit[int(best)]) and float(fit[int(best)]) >= 0.4       # 40 % of the rows have a counterpart
    truth = dev(ec.pose44(a["C"], a["r"], np.float32))
    fit_t, _, _ = evaluate_registration(x, y, truth, dist)
    assert float(fit1) >= float(fit_t) - 0.01                                            # ... and ICP ends as good as the true pose


# ------------------------------------------------------------------ 6: other input forms
@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_tensors_and_single_pair_forms(dtype):
    c = batch(257, 5, dtype)
    x, y, T = (torch.from_numpy(c[k]) for k in ("x", "y", "T"))
    srows, trows = (torch.tensor(c[k]) for k in ("srows", "trows"))
    on_cpu = evaluate_registration(x, y, T, c["radius"], srows, trows, return_correspondences=True)
    on_dev = evaluate_registration(x.cuda(), y.cuda(), T.cuda(), c["radius"], srows.cuda(), trows.cuda(), return_correspondences=True)
    assert not any(t.is_cuda for t in on_cpu) and all(same(a.cuda(), b) for a, b in zip(on_cpu, on_dev))
    info_cpu = information_matrix(x, y, T, c["radius"], srows, trows)
    assert not info_cpu.is_cuda and info_cpu.shape == (3, 5, 6, 6) and info_cpu.dtype == torch.float64
    for b in range(3):
        for h in range(5):
            L = host(info_cpu[b, h])
            assert np.array_equal(L, er.assemble(c["ref"][b]["sums"][h], c["ref"][b]["counts"][h])) and np.array_equal(L, L.T)     # (== : the sign of a zero is free)
            plain, bound = ec.info_bound(c["y"][b], c["ref"][b]["idx"][h])
            assert np.all(np.abs(L - plain) <= bound) and np.array_equal(L[3:, 3:], float(c["ref"][b]["counts"][h]) * np.eye(3))
    assert not host(info_cpu[2]).any()                                                  # a source without rows: zero matrices
    # one pair: (H, 4, 4) and (4, 4) against cloud 1 of the batch cut to its rows
    xs, ys = x[1, :c["srows"][1]].cuda(), y[1, :c["trows"][1]].cuda()
    many = evaluate_registration(xs, ys, T[1].cuda(), c["radius"], return_correspondences=True)
    assert [tuple(t.shape) for t in many] == [(5,), (5,), (5,), (5, c["srows"][1]), (5, c["srows"][1])]
    for a, b in zip(many[:3], on_dev[:3]):
        assert same(a, b[1])
    assert same(many[3], on_dev[3][1, :, :c["srows"][1]]) and same(many[4], on_dev[4][1, :, :c["srows"][1]])
    one = evaluate_registration(xs, ys, T[1, 3].cuda(), c["radius"], return_correspondences=True)
    assert [tuple(t.shape) for t in one] == [(), (), (), (c["srows"][1],), (c["srows"][1],)]
    assert all(same(a, b[3]) for a, b in zip(one, many))
    assert information_matrix(xs, ys, T[1, 3].cuda(), c["radius"]).shape == (6, 6) and information_matrix(xs, ys, T[1].cuda(), c["radius"]).shape == (5, 6, 6)
    r_dev = torch.tensor(c["radius"], dtype=torch.float64).cuda()                       # a 0-d device tensor is not read back
    assert all(same(a, b) for a, b in zip(evaluate_registration(xs, ys, T[1].cuda(), r_dev), many[:3]))
    empty = evaluate_registration(xs[:0], ys, T[1].cuda(), c["radius"], return_correspondences=True)
    assert empty[3].shape == (5, 0) and not bool(empty[2].any()) and not bool(empty[0].any())
    none = evaluate_registration(xs, ys[:0], T[1].cuda(), c["radius"])
    assert not bool(none[2].any()) and not bool(none[0].any()) and not bool(none[1].any())


def test_a_call_in_a_captured_graph():
    def data(seed):
        c = [ec.magnitudes_case(seed + b, 300, M, 3, np.float32) for b in range(2)]
        return {"x": dev(np.stack([v[0] for v in c])), "y": dev(np.stack([v[1] for v in c])), "T": dev(np.stack([v[2] for v in c]))}

    rows = torch.tensor([300, 270], dtype=torch.int32).cuda()

    def run(s):
        out = evaluate_registration(s["x"], s["y"], s["T"], 0.05, source_rows=rows, return_correspondences=True)
        return out + (information_matrix(s["x"], s["y"], s["T"], 0.05, source_rows=rows),) + best_pose(s["T"], out[2], out[1])
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
        assert len(eager) == len(captured) and all(same(a, b) for a, b in zip(captured, eager)), seed
        assert bool((eager[2] > 0).any())
