"""second_order_compatibility / prune_correspondences(order=2) / consensus_correspondences on the MI355X (dicp_amd/compat.py, register.py;
csrc/compat2.hip), against the numpy restatement tests/compat2_ref.py.

1  every stage at the edges of the kernels' tiles -- P in {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025} with
   n = P and n = P + 70, both dtypes: adj word for word (every zero pad bit), degree, degree2, rank2, the member lists, counts, best,
   best_count, the inlier sets exactly, score2 and pose_best bit for bit, the reference evaluated on the kernel's own stored poses; the
   stored poses against float64 Kabsch inside the bound of profiles/r30_consensus_edges.txt;
2  a ragged batch of three clouds whose pad rows hold NaN and whose idx holds -1 and out-of-range values, rows with a non-finite
   coordinate; exact duplicates with min_length 0 and > 0; a complete graph, an empty one, a clique plus isolated rows; seeds > P and
   members > the candidates;
3  the public functions: the outputs in the original row order, order=2 pruning element for element, order=1 the bytes of
   correspondence_compatibility's own path, three repeated calls, a captured graph, the gradients of T;
4  the recovery case at 18 true matches of 600.
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import match as M
from dicp_amd.match import (align_correspondences, consensus_correspondences, correspondence_compatibility, prune_correspondences,
                            ransac_correspondences, second_order_compatibility)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compat2_cases as cc  # noqa: E402
import compat2_ref as c2  # noqa: E402
import compat_ref as cr  # noqa: E402
import ransac_cases as rc  # noqa: E402
import ransac_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
P_CASES = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025)
TAU = 0.03
INT_MAX = 0x7fffffff


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def stages(x, y, idx, seeds, members, refine, weight=None, x_rows=None, min_length=0.0, thr=TAU, thr_in=None):
    """_consensus_stages on numpy inputs (batches)"""
    rows = None if x_rows is None else torch.tensor(x_rows, dtype=torch.int32).cuda()
    _, _, xd, yd, idx_d, w, rows_d = M._pair_arguments(dev(x), dev(y), dev(idx), None if weight is None else dev(weight), rows, "test")
    return M._consensus_stages(xd, yd, idx_d, w, rows_d, thr, thr if thr_in is None else thr_in, seeds, members, refine, min_length)


def check_stages(st, x, y, idx, seeds, members, refine, x_rows=None, min_length=0.0, thr=TAU, thr_in=None, weight=None):
    """every stage of every cloud against the restatement evaluated on the kernel's own poses -> the restatements"""
    refs = []
    for b in range(x.shape[0]):
        dtype = x.dtype.type
        n = x.shape[1]
        rows_b = None if x_rows is None else x_rows[b]
        poses = host(st["poses"][b])
        ref = c2.consensus_ref(x[b], y[b], idx[b], thr, thr_in, seeds, members, refine, None if weight is None else weight[b], min_length, rows_b,
                               poses=poses, round_poses=[host(p[b]) for p in st["round_poses"]])
        P = ref["P"]
        assert int(st["P"][b]) == P, b
        assert np.array_equal(host(st["live"][b]), rr.live_mask(x[b], y[b], idx[b], rows_b))
        assert rc.same_bits(host(st["pairs"][b, :P]), ref["pairs"])
        assert np.array_equal(host(st["adj"][b]), ref["adj"]), b                                   # every word, the zero pad bits included
        assert np.array_equal(host(st["degree_packed"][b, :P]), ref["degree_packed"]) and not host(st["degree_packed"][b, P:]).any()
        assert np.array_equal(host(st["degree2_packed"][b, :P]), ref["degree2_packed"]) and not host(st["degree2_packed"][b, P:]).any()
        assert np.array_equal(host(st["rank2_packed"][b, :P]), ref["rank2_packed"]) and (host(st["rank2_packed"][b, P:]) == INT_MAX).all()
        assert rc.same_bits(host(st["score2_packed"][b, :P]), ref["score2_packed"]) and not host(st["score2_packed"][b, P:]).any()
        assert rc.same_bits(host(st["score2"][b]), ref["score2"]) and np.array_equal(host(st["degree2"][b]), ref["degree2"])
        assert np.array_equal(host(st["degree"][b]), ref["degree"])
        assert np.array_equal(host(st["members"][b]), ref["members"]), b
        assert np.array_equal(host(st["real"][b]), ref["real"])
        assert np.array_equal(poses[~ref["real"]], np.tile(rr.IDENTITY.astype(dtype), (int((~ref["real"]).sum()), 1)))
        ok, count, wc, wr = c2.poses_hold(poses, ref["pairs"], ref["members"])
        print("cloud %d %s n %d P %d: %d real hypotheses, %d poses compared, worst dC / bound %.3g, worst dr / bound %.3g"
              % (b, np.dtype(dtype).name, n, P, int(ref["real"].sum()), count, wc, wr))
        assert ok, (b, wc, wr)
        assert np.array_equal(host(st["counts"][b]), ref["counts"]), b
        assert int(st["best"][b]) == ref["best"] and int(st["best_count"][b]) == ref["best_count"], b
        assert rc.same_bits(host(st["pose_best"][b]), ref["pose_best"])
        for j, (got, want) in enumerate(zip(st["sets"], ref["sets"])):
            assert np.array_equal(host(got[b]), want), (b, j)
        assert np.array_equal(host(st["inliers"][b]), ref["inliers"])
        refs.append(ref)
    return refs


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", P_CASES)
def test_tile_edges(dtype, P):
    for extra in (0, 70):
        n = max(P + extra, 1)
        rng = np.random.default_rng(P + extra)
        x, y, idx = cc.motion_cloud(rng, n, n + 9, P, dtype, inliers=max(P // 4, 6))
        st = stages(x[None], y[None], idx[None], 40, 12, 1)
        ref = check_stages(st, x[None], y[None], idx[None], 40, 12, 1)[0]
        if P >= 63:
            assert ref["real"].sum() >= 4 and ref["best_count"] >= 6


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_batch_with_poisoned_padding(dtype):
    rng = np.random.default_rng(11)
    rows = [300, 251, 130]
    cs = [cc.motion_cloud(rng, 300, 340, P, dtype, inliers=30, rows=r) for P, r in zip((260, 200, 64), rows)]
    x, y, idx = (np.stack([c[k] for c in cs]) for k in range(3))
    w = rng.uniform(0.5, 1.5, (3, 300)).astype(dtype)
    for b, r in enumerate(rows):
        w[b, r:] = np.nan
    for weight, refine in ((None, 0), (w, 2)):
        st = stages(x, y, idx, 64, 16, refine, weight=weight, x_rows=rows, thr_in=0.05)
        refs = check_stages(st, x, y, idx, 64, 16, refine, x_rows=rows, thr_in=0.05, weight=weight)
        for ref in refs:
            assert ref["best_count"] >= 25                      # the motion is found


def designed(dtype):
    """-> x, y, idx (4, 40, ...): a complete graph, exact duplicates, a clique of 10 plus isolated rows, two rows"""
    rng = np.random.default_rng(4)
    x = np.tile(rng.uniform(0, 1, (40, 3))[None], (4, 1, 1))
    y = x + 0.25
    x[1], y[1] = x[1, :1], y[1, :1]
    y[2, 10:] = rng.uniform(0, 50, (30, 3)) * np.arange(1, 31)[:, None]
    idx = np.tile(np.arange(40)[None], (4, 1))
    idx[3, 2:] = -1
    return x.astype(dtype), y.astype(dtype), idx.astype(np.int64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_designed_graphs(dtype):
    x, y, idx = designed(dtype)
    for L in (0.0, 1e-6):
        st = stages(x, y, idx, 48, 32, 1, min_length=L, thr=0.01)            # seeds > P, members > the candidates
        check_stages(st, x, y, idx, 48, 32, 1, min_length=L, thr=0.01)
        d1, d2, mem = host(st["degree_packed"]), host(st["degree2_packed"]), host(st["members"])
        assert (d1[0] == 39).all() and (d2[0] == 39 * 38).all() and np.array_equal(mem[0, 3, :5], [3, 0, 1, 2, 4]) and (mem[0, 40:] == -1).all()
        assert (d1[1] == (39 if L == 0.0 else 0)).all() and (d2[1] == (39 * 38 if L == 0.0 else 0)).all()
        assert (d2[2, :10] == 72).all() and not d2[2, 10:].any() and np.array_equal(mem[2, 2, :11], [2, 0, 1, 3, 4, 5, 6, 7, 8, 9, -1])
        assert np.array_equal(mem[2, 10], [10] + [-1] * 31) and int(st["best_count"][2]) == 10
        assert int(st["best"][3]) == -1 and not host(st["inliers"][3]).any() and np.array_equal(mem[3, :2, :2], [[0, -1], [1, -1]])
        if L > 0:                                               # an empty graph with P >= 3: no real hypothesis, the identity, count 0
            assert not host(st["real"][1]).any() and int(st["best"][1]) == 0 and int(st["best_count"][1]) == 0


# ------------------------------------------------------------------ 3
def public_case(dtype):
    rng = np.random.default_rng(21)
    rows = [400, 333]
    cs = [cc.motion_cloud(rng, 400, 450, P, dtype, inliers=40, rows=r) for P, r in zip((350, 280), rows)]
    x, y, idx = (np.stack([c[k] for c in cs]) for k in range(3))
    return x, y, idx, rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_public_functions(dtype):
    x, y, idx, rows = public_case(dtype)
    xd, yd, id_, rw = dev(x), dev(y), dev(idx), torch.tensor(rows, dtype=torch.int32).cuda()
    runs = [second_order_compatibility(xd, yd, id_, TAU, x_rows=rw, return_adjacency=True) + prune_correspondences(xd, yd, id_, TAU, 50, x_rows=rw, order=2)
            + consensus_correspondences(xd, yd, id_, TAU, inlier_threshold=0.05, x_rows=rw, return_hypothesis=True) for _ in range(3)]
    for r in runs[1:]:                                          # the same bytes on every run
        for a, b in zip(runs[0], r):
            assert a.dtype == b.dtype and rc.same_bits(host(a), host(b))
    s2, d2, d1, adj, kept, s2k, T, inl, best, bc, Tb, mem = runs[0]
    assert s2.dtype == xd.dtype and d2.dtype == torch.int64 and d1.dtype == torch.int32 and adj.dtype == torch.int64 and adj.shape == (2, 400, 7)
    for b in range(2):
        ref = c2.consensus_ref(x[b], y[b], idx[b], TAU, 0.05, 64, 16, 0, x_rows=rows[b])
        full = c2.compat2_ref(x[b], y[b], idx[b], TAU, x_rows=rows[b], keep=50)
        assert rc.same_bits(host(s2[b]), full["score2"]) and np.array_equal(host(d2[b]), full["degree2"]) and np.array_equal(host(d1[b]), full["degree"])
        assert np.array_equal(host(adj[b]), full["adj"]) and np.array_equal(host(kept[b]), full["idx_kept"]) and rc.same_bits(host(s2k[b]), full["score2"])
        assert int((host(kept[b]) >= 0).sum()) == 50 and np.array_equal(host(mem[b]), ref["members"])
        # a single cloud gives the batch's rows
        one = second_order_compatibility(xd[b, :rows[b]], yd[b], id_[b, :rows[b]], TAU)
        assert one[0].shape == (rows[b],) and rc.same_bits(host(one[0]), full["score2"][:rows[b]]) and np.array_equal(host(one[1]), full["degree2"][:rows[b]])
        T1, inl1 = consensus_correspondences(xd[b, :rows[b]], yd[b], id_[b, :rows[b]], TAU, inlier_threshold=0.05)
        assert T1.shape == (4, 4) and torch.equal(inl1, inl[b, :rows[b]])
    # order=1 is today's path: the bytes of correspondence_compatibility and of its own ranks
    k1, s1 = prune_correspondences(xd, yd, id_, TAU, 50, x_rows=rw)
    k1b, s1b = prune_correspondences(xd, yd, id_, TAU, 50, x_rows=rw, order=1)
    sc, _ = correspondence_compatibility(xd, yd, id_, TAU, x_rows=rw)
    _, _, xa, ya, ia, _, ra = M._pair_arguments(xd, yd, id_, None, rw, "test")
    st1 = M._compat_stages(xa, ya, ia, ra, TAU, 10, 0.0, keep=50)
    assert rc.same_bits(host(s1), host(sc)) and rc.same_bits(host(s1b), host(sc)) and torch.equal(k1, k1b) and torch.equal(k1, st1["idx_kept"])
    # CPU tensors are computed on the GPU and returned on the CPU
    in_range = np.minimum(idx, y.shape[1] - 1)                  # (an idx at or past m on the CPU is a ValueError; those rows are padding)
    c = second_order_compatibility(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(in_range), TAU, x_rows=torch.tensor(rows, dtype=torch.int32))
    assert not c[0].is_cuda and rc.same_bits(host(c[0]), host(s2)) and torch.equal(c[1], d2.cpu())


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients_are_those_of_the_final_fit(dtype):
    x, y, idx, rows = public_case(dtype)
    rng = np.random.default_rng(5)
    w = rng.uniform(0.5, 1.5, idx.shape).astype(dtype)
    rw = torch.tensor(rows, dtype=torch.int32).cuda()
    g = dev(rng.standard_normal((2, 4, 4)).astype(dtype))
    outs = []
    for fit in (False, True):
        xd, yd, wd = (dev(np.nan_to_num(t, nan=0.5, posinf=0.5)).requires_grad_() for t in (x, y, w))
        if fit:
            T = align_correspondences(xd, yd, torch.where(outs[0][4], dev(idx), torch.full_like(dev(idx), -1)), weight=wd, x_rows=rw)
            inl = outs[0][4]
        else:
            T, inl = consensus_correspondences(xd, yd, dev(idx), TAU, inlier_threshold=0.05, weight=wd, x_rows=rw)
            assert not inl.requires_grad and T.requires_grad
        (T * g).sum().backward()
        outs.append((T.detach(), xd.grad, yd.grad, wd.grad, inl))
    for a, b in zip(outs[0][:4], outs[1][:4]):
        assert rc.same_bits(host(a), host(b))
    assert float(outs[0][1].abs().sum()) > 0 and int(outs[0][4].sum()) >= 60


def test_captured_call():
    def data(seed):
        rng = np.random.default_rng(seed)
        rows = [500, 444]
        cs = [cc.motion_cloud(rng, 500, 520, P, np.float32, inliers=35, rows=r) for P, r in zip((430, 3), rows)]
        x, y, idx = (np.stack([c[k] for c in cs]) for k in range(3))
        return {"x": dev(x), "y": dev(y), "idx": dev(idx), "rows": torch.tensor(rows, dtype=torch.int32).cuda()}

    def run(s):
        return consensus_correspondences(s["x"], s["y"], s["idx"], TAU, inlier_threshold=0.05, seeds=32, members=10, x_rows=s["rows"], return_hypothesis=True)
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
    fresh = data(2)
    for key, t in fresh.items():
        static[key].copy_(t)
    graph.replay()
    torch.cuda.synchronize()
    eager = run(fresh)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(captured, eager)):
        assert rc.same_bits(host(a), host(b)), i
    assert int(captured[3][0]) >= 30


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("dtype", DTYPES)
def test_recovery_case(dtype):
    for seed in range(5):
        a = cr.recovery_case(seed, n=600, inliers=18, dtype=dtype)
        st = stages(a["x"][None], a["y"][None], a["idx"][None], 32, 10, 0, thr=0.05)
        ref = check_stages(st, a["x"][None], a["y"][None], a["idx"][None], 32, 10, 0, thr=0.05)[0]        # (on the kernel's own poses)
        x, y, idx = dev(a["x"]), dev(a["y"]), dev(a["idx"])
        T, inl, best, bc, Tb, mem = consensus_correspondences(x, y, idx, 0.05, seeds=32, members=10, refine=0, return_hypothesis=True)
        _, inl_r = ransac_correspondences(x, y, idx, 0.05, hypotheses=64, seed=7, refine=0)
        err_ref = cr.rotation_angle(ref["pose"][:9], a["C"])
        err = cr.rotation_angle(host(T[:3, :3]).reshape(-1), a["C"])
        print("seed %d %s: consensus %d inliers (%d true) %.3g rad, the restatement %.3g rad; ransac H = 64 on the unpruned matches: %d inliers (%d true)"
              % (seed, np.dtype(dtype).name, int(inl.sum()), int(inl[dev(a["truth"])].sum()), err, err_ref, int(inl_r.sum()), int(inl_r[dev(a["truth"])].sum())))
        assert np.array_equal(host(mem[0]), ref["members"]) and int(best[0]) == ref["best"] and int(bc[0]) == ref["best_count"]
        assert np.array_equal(host(inl), ref["inliers"])
        assert host(inl)[a["truth"]].all()
        assert err_ref < 5e-3                                   # the restatement's own float64 fit on the inliers
