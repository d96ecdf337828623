"""correspondence_compatibility / prune_correspondences on the MI355X (dicp_amd/compat.py; csrc/compat.hip), against the numpy restatement
tests/compat_ref.py.

1  score, degree and idx_kept bit for bit in float32 and float64: P at and around every edge of the kernel's block (R rows) and tile (S rows)
   -- P in {1, 2, 3, R - 1, R, R + 1, S - 1, S, S + 1, 2 S + 76}, R and S from dicp_compat_geometry -- as one ragged batch, iterations in
   {0, 1, 2, 10}, min_length 0 and positive, keep in {1, P - 1, P, n + 5} for every P; the designed tables of tests/compat_cases.py;
2  a ragged batch of three clouds with x_rows (0, 257, n), int32 and int64 idx, pad rows holding NaN, 1e30 and indices out of range,
   against the per-cloud single calls;
3  three runs give the same bytes; the relation is symmetric (x and y swapped);
4  both functions in a captured graph;  5  the recovery case: prune -> RANSAC with 64 hypotheses -> ICP.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import _lib
from dicp_amd.ICP import ICP
from dicp_amd.match import correspondence_compatibility, prune_correspondences, ransac_correspondences

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compat_cases as cc  # noqa: E402
import compat_ref as cr  # noqa: E402
import ransac_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

TD = {np.float32: torch.float32, np.float64: torch.float64}
DTYPES = [np.float32, np.float64]
ITERATIONS = (0, 1, 2, 10)
LENGTHS = (0.0, 0.5)
same_bits = cc.same_bits


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def geometry():
    rows, tile = ctypes.c_int32(), ctypes.c_int32()
    _lib.load().dicp_compat_geometry(ctypes.byref(rows), ctypes.byref(tile))
    return rows.value, tile.value


def edge_sizes():
    R, S = geometry()
    return sorted({1, 2, 3, R - 1, R, R + 1, S - 1, S, S + 1, 2 * S + 76})


_EDGE = {}


def edge_batch(dtype):
    """one ragged batch with a cloud per edge size, and per min_length the restatement of every cloud through 10 iterations (computed
    once, shared by the tests, never changed)"""
    if dtype not in _EDGE:
        Ps = edge_sizes()
        n = max(Ps) + 40
        rng = np.random.default_rng(7)
        rows = [min(n, P + 20 + 3 * k) for k, P in enumerate(Ps)]
        cs = [cc.cloud(rng, n, n + 30, P, dtype, rows=r) for P, r in zip(Ps, rows)]
        x, y, idx = (np.stack([c[k] for c in cs]) for k in range(3))
        refs = {}
        for L in LENGTHS:
            per = []
            for b, P in enumerate(Ps):
                live, pairs = rr.packed(x[b], y[b], idx[b], rows[b])
                assert live.size == P
                rel = cr.relation(pairs, cc.TAU, L)["rel"]
                ws, vs = cr.power(rel, max(ITERATIONS), dtype)
                per.append(dict(rows=live, deg=cr.degree_of(rel), vs=vs))
            refs[L] = per
        _EDGE[dtype] = dict(Ps=Ps, n=n, rows=rows, x=x, y=y, idx=idx, refs=refs,
                            dev=(dev(x), dev(y), dev(idx), torch.tensor(rows, dtype=torch.int32).cuda()))
    return _EDGE[dtype]


def expected(ref, n, iterations, dtype):
    """score (n,), degree (n,), packed score of one cloud of the edge batch after `iterations`"""
    sp = ref["vs"][iterations - 1] if iterations else np.ones(ref["rows"].size, dtype=dtype)
    score, degree = np.zeros(n, dtype=dtype), np.zeros(n, dtype=np.int32)
    score[ref["rows"]], degree[ref["rows"]] = sp, ref["deg"]
    return score, degree, sp


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("iterations", ITERATIONS)
def test_bit_for_bit_at_the_tile_edges(dtype, L, iterations):
    e = edge_batch(dtype)
    R, S = geometry()
    assert {R - 1, R, R + 1, S - 1, S, S + 1} <= set(e["Ps"]) and max(e["Ps"]) > 2 * S
    xd, yd, id_, rw = e["dev"]
    n = e["n"]
    score, degree = correspondence_compatibility(xd, yd, id_, cc.TAU, iterations=iterations, min_length=L, x_rows=rw)
    assert score.shape == (len(e["Ps"]), n) and score.dtype == TD[dtype] and degree.dtype == torch.int32
    assert not score.requires_grad and not degree.requires_grad
    want = [expected(ref, n, iterations, dtype) for ref in e["refs"][L]]
    for b, P in enumerate(e["Ps"]):
        assert np.array_equal(host(degree[b]), want[b][1]), (P, "degree")
        assert same_bits(host(score[b]), want[b][0]), (P, "score")
    if iterations == 1:                                         # w^1 = degree + 1 exactly: score = (degree + 1) / max
        b = len(e["Ps"]) - 1
        d1 = (want[b][1][e["refs"][L][b]["rows"]] + 1).astype(dtype)
        assert same_bits(want[b][2], (d1 / d1.max()).astype(dtype))
    keeps = sorted({1, n + 5} | set(e["Ps"]) | {P - 1 for P in e["Ps"] if P > 1})
    for keep in keeps:
        idx_kept, s2 = prune_correspondences(xd, yd, id_, cc.TAU, keep, iterations=iterations, min_length=L, x_rows=rw)
        assert idx_kept.dtype == torch.int64 and idx_kept.shape == id_.shape and torch.equal(s2, score)
        got = host(idx_kept)
        for b, P in enumerate(e["Ps"]):
            if keep not in (1, n + 5, P - 1, P):
                continue
            ref = e["refs"][L][b]
            kept = np.zeros(n, dtype=bool)
            kept[ref["rows"][cr.ranks(want[b][2]) < keep]] = True
            assert np.array_equal(got[b], np.where(kept, e["idx"][b], -1)), (P, keep)
            assert kept.sum() == min(keep, P)


@pytest.mark.parametrize("dtype", DTYPES)
def test_designed_tables_through_the_kernels(dtype):
    tabs = cc.edge_tables(dtype) + [cc.few_pairs(dtype, P) for P in range(4)]
    for tb in tabs:
        for it in (0, 3):
            ref = cr.compat_ref(tb["x"], tb["y"], tb["idx"], tb["threshold"], it, tb["min_length"], keep=2)
            score, degree = correspondence_compatibility(dev(tb["x"]), dev(tb["y"]), dev(tb["idx"]), tb["threshold"], iterations=it, min_length=tb["min_length"])
            kept, _ = prune_correspondences(dev(tb["x"]), dev(tb["y"]), dev(tb["idx"]), tb["threshold"], 2, iterations=it, min_length=tb["min_length"])
            assert same_bits(host(score), ref["score"]), tb["name"]
            assert np.array_equal(host(degree), ref["degree"]), tb["name"]
            assert np.array_equal(host(kept), ref["idx_kept"]), tb["name"]
    # CPU tensors: computed on the GPU, returned on the CPU
    tb = tabs[0]
    ref = cr.compat_ref(tb["x"], tb["y"], tb["idx"], tb["threshold"], 3, keep=3)
    s, d = correspondence_compatibility(torch.from_numpy(tb["x"]), torch.from_numpy(tb["y"]), torch.from_numpy(tb["idx"]), tb["threshold"], iterations=3)
    k, _ = prune_correspondences(torch.from_numpy(tb["x"]), torch.from_numpy(tb["y"]), torch.from_numpy(tb["idx"]), tb["threshold"], 3, iterations=3)
    assert not s.is_cuda and not d.is_cuda and not k.is_cuda
    assert same_bits(s.numpy(), ref["score"]) and np.array_equal(d.numpy(), ref["degree"]) and np.array_equal(k.numpy(), ref["idx_kept"])
    # idx at or past m on a device tensor: clamped to the last row of y
    tb = [t for t in tabs if t["name"] == "not_live"][0]
    big = tb["idx"].copy()
    big[2], big[4] = 11, 6
    ref = cr.compat_ref(tb["x"], tb["y"], big, tb["threshold"], 3, keep=2)
    assert ref["P"] == 3
    s, d = correspondence_compatibility(dev(tb["x"]), dev(tb["y"]), dev(big), tb["threshold"], iterations=3)
    k, _ = prune_correspondences(dev(tb["x"]), dev(tb["y"]), dev(big), tb["threshold"], 2, iterations=3)
    assert same_bits(host(s), ref["score"]) and np.array_equal(host(d), ref["degree"]) and np.array_equal(host(k), ref["idx_kept"])


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_batch_equals_single_calls(dtype):
    rng = np.random.default_rng(31)
    n, m = 300, 340
    rows = [0, 257, n]
    cs = [cc.cloud(rng, n, m, P, dtype, rows=r) for P, r in zip((0, 200, 270), rows)]
    x, y, idx = (np.stack([c[k] for c in cs]) for k in range(3))
    assert np.isnan(x[1, 257:]).any() and (x[1, 257:] == dtype(1e30)).any() and (idx[1, 257:] >= m).any() and (idx[1, 257:] < 0).any()
    rw = torch.tensor(rows).cuda()
    for it_dtype in (np.int64, np.int32):
        id_ = dev(idx.astype(it_dtype))
        score, degree = correspondence_compatibility(dev(x), dev(y), id_, cc.TAU, iterations=5, min_length=0.25, x_rows=rw)
        kept, s2 = prune_correspondences(dev(x), dev(y), id_, cc.TAU, 100, iterations=5, min_length=0.25, x_rows=rw)
        assert kept.dtype == id_.dtype and torch.equal(s2, score)
        for b, r in enumerate(rows):
            ref = cr.compat_ref(x[b], y[b], idx[b].astype(it_dtype), cc.TAU, 5, 0.25, x_rows=r, keep=100)
            assert same_bits(host(score[b]), ref["score"]) and np.array_equal(host(degree[b]), ref["degree"]) and np.array_equal(host(kept[b]), ref["idx_kept"])
            assert not host(score[b, r:]).any() and not host(degree[b, r:]).any() and np.all(host(kept[b, r:]) == -1)
            if r == 0:
                continue
            s1, d1 = correspondence_compatibility(dev(x[b, :r]), dev(y[b]), id_[b, :r], cc.TAU, iterations=5, min_length=0.25)
            k1, _ = prune_correspondences(dev(x[b, :r]), dev(y[b]), id_[b, :r], cc.TAU, 100, iterations=5, min_length=0.25)
            assert s1.shape == (r,) and same_bits(host(s1), host(score[b, :r])) and torch.equal(d1, degree[b, :r]) and torch.equal(k1, kept[b, :r])
        assert int((kept[2] >= 0).sum()) == 100 and int((kept[1] >= 0).sum()) == 100


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("dtype", DTYPES)
def test_repeatable_and_symmetric(dtype):
    e = edge_batch(dtype)
    xd, yd, id_, rw = e["dev"]
    runs = [prune_correspondences(xd, yd, id_, cc.TAU, 300, iterations=10, x_rows=rw) + correspondence_compatibility(xd, yd, id_, cc.TAU, x_rows=rw)
            for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert same_bits(host(a), host(b))
    # x and y swapped: the matched target points as the source, the source points as the target, idx the identity where the row is live
    N, n = id_.shape
    m = yd.shape[1]
    yg = torch.gather(yd, 1, id_.clamp(min=0, max=m - 1)[..., None].expand(N, n, 3))
    ident = torch.where(id_ >= 0, torch.arange(n, device=id_.device)[None, :].expand(N, n), torch.full_like(id_, -1))
    s_sw, d_sw = correspondence_compatibility(yg, xd, ident, cc.TAU, x_rows=rw)
    assert torch.equal(d_sw, runs[0][3]) and same_bits(host(s_sw), host(runs[0][2]))
    assert int(runs[0][3].max()) > 10


# ------------------------------------------------------------------ 4
def test_captured_calls():
    def data(seed):
        rng = np.random.default_rng(seed)
        rows = [600, 600, 555]
        cs = [cc.cloud(rng, 600, 640, P, np.float32, rows=r) for P, r in zip((530, 3, 300), rows)]
        x, y, idx = (np.stack([c[k] for c in cs]) for k in range(3))
        return {"x": dev(x), "y": dev(y), "idx": dev(idx), "rows": torch.tensor(rows, dtype=torch.int32).cuda()}

    def run(s):
        return (correspondence_compatibility(s["x"], s["y"], s["idx"], cc.TAU, iterations=4, x_rows=s["rows"])
                + prune_correspondences(s["x"], s["y"], s["idx"], cc.TAU, 50, iterations=10, min_length=0.1, x_rows=s["rows"]))
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
            assert same_bits(host(a), host(b)), (seed, i)
        assert int((captured[2] >= 0).sum()) == 50 + 3 + 50


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("seed", range(5))
def test_recovery_case(seed):
    a = cr.recovery_case(seed)
    ref = cr.compat_ref(a["x"], a["y"], a["idx"], cc.TAU, 10, keep=60)
    x, y, idx = dev(a["x"]), dev(a["y"]), dev(a["idx"])
    idx_kept, score = prune_correspondences(x, y, idx, cc.TAU, 60)
    assert np.array_equal(host(idx_kept), ref["idx_kept"]) and same_bits(host(score), ref["score"])     # the kept set, index for index
    T0, inl = ransac_correspondences(x, y, idx_kept, 3 * cc.TAU, hypotheses=64, seed=cc.RANSAC_SEED)
    kept_true = dev(ref["kept"] & a["truth"])
    assert bool(inl[kept_true].all())
    # ICP of the source points RANSAC kept against the whole target, from RANSAC's pose
    out = ICP(icp_type="pt2pt", max_iterations=20, tolerance=1e-9).icp(x[inl][None], y[None], T_init=T0[None])
    err0 = cr.rotation_angle(host(T0[:3, :3]).reshape(-1), a["C"])
    err = cr.rotation_angle(host(out["T"][0, :3, :3]).reshape(-1), a["C"])
    print("case %d: %d of 60 kept are true, RANSAC %d inliers %.3g rad, after ICP %.3g rad" % (seed, int(kept_true.sum()), int(inl.sum()), err0, err))
    assert err < 1e-3
    _, inl_plain = ransac_correspondences(x, y, idx, 3 * cc.TAU, hypotheses=64, seed=cc.RANSAC_SEED)
    assert int(inl_plain.sum()) < int(a["truth"].sum())       # the same H and seed on every match do not find the motion
