"""CPU checks of second_order_compatibility / prune_correspondences(order=2) / consensus_correspondences (dicp_amd/compat.py, register.py) that need no
GPU.

1  the g++ build of csrc/dicp_compat2.h (tests/hostcheck/compat2_check.cpp: the lines the kernels run) against the numpy restatement
   tests/compat2_ref.py: the bits word for word, S, degree2, rank2, score2 and the member lists exactly, the sums of a list bit for bit,
   the pose of a list inside the bound of profiles/r30_consensus_edges.txt; every deliberately wrong restatement fails the same comparison;
2  the claim the feature rests on, on the restatement: at 18 true matches of 600 the second-order degree separates them where the
   first-order degree does not, and the seeded consensus finds all of them;
3  the argument checks of the Python functions.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compat2_cases as cc  # noqa: E402
import compat2_ref as c2  # noqa: E402
import compat_ref as cr  # noqa: E402
import ransac_cases as rc  # noqa: E402
import ransac_ref as rr  # noqa: E402
from dicp_amd.match import consensus_correspondences, prune_correspondences, second_order_compatibility  # noqa: E402

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def check():
    return cc.build()


def cloud_pairs(seed, P, dtype, inliers):
    rng = np.random.default_rng(seed)
    x, y, idx = cc.motion_cloud(rng, P, P + 5, P, dtype, inliers)
    return rr.packed(x, y, idx)[1], (x, y, idx)


def compare(h, ref, lists, n, P):
    """the host build's stages against a restatement's: the names of the stages that differ"""
    bad = []
    if not np.array_equal(h["adj"], ref["adj"]):
        bad.append("adj")
    if not np.array_equal(h["degree"][:P], ref["degree_packed"]) or h["degree"][P:].any():
        bad.append("degree")
    if not np.array_equal(h["S"].astype(np.int64), ref["S"]):
        bad.append("S")
    if not np.array_equal(h["degree2"], ref["degree2_packed"]):
        bad.append("degree2")
    if not np.array_equal(h["rank2"], ref["rank2_packed"]):
        bad.append("rank2")
    if not rc.same_bits(h["score2"], ref["score2_packed"]):
        bad.append("score2")
    if not np.array_equal(h["lists"], lists):
        bad.append("lists")
    return bad


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,extra", [(0, 5), (1, 0), (2, 70), (3, 0), (63, 0), (64, 0), (65, 70), (130, 0), (200, 70)])
def test_header_matches_restatement(check, dtype, P, extra):
    n = P + extra
    pairs, (x, y, idx) = cloud_pairs(P + extra, max(P, 1), dtype, inliers=max(P // 3, 3))
    pairs = pairs[:P]
    seeds, members = 12, 7
    h = cc.header_stages(check, pairs, n, 0.03, 0.0, seeds, members)
    M = c2.adjacency(cr.relation(pairs, 0.03, 0.0)["rel"])
    S, d2 = c2.second_order(M)
    ref = dict(adj=c2.bits(M, n), degree_packed=M.sum(axis=1).astype(np.int32), S=S, degree2_packed=d2, rank2_packed=c2.ranks2(d2),
               score2_packed=c2.score2_of(d2, dtype))
    lists = c2.member_lists(S, ref["rank2_packed"], seeds, members)
    assert compare(h, ref, lists, n, P) == []
    assert np.array_equal(c2.unpack(h["adj"], P), M) and np.array_equal(c2.popcount(h["adj"]).sum(axis=1)[:P], ref["degree_packed"])
    assert np.array_equal(M, M.T)                               # symmetric bit for bit
    for k in range(seeds):                                      # the sums in member order, bit for bit
        lst = lists[k][lists[k] >= 0]
        assert rc.same_bits(h["sums"][k], c2.list_sums(pairs, lst)), k
        if lst.size < 3:
            assert np.array_equal(h["poses"][k], rr.IDENTITY.astype(dtype))
    ok, count, wc, wr = c2.poses_hold(h["poses"], pairs, lists)
    print("P %d %s: %d lists compared, worst dC / bound %.3g, worst dr / bound %.3g" % (P, np.dtype(dtype).name, count, wc, wr))
    assert ok


@pytest.mark.parametrize("dtype", DTYPES)
def test_wrong_restatements_are_refused(check, dtype):
    P, n, seeds, members = 150, 190, 16, 6
    pairs, _ = cloud_pairs(7, P, dtype, inliers=40)
    h = cc.header_stages(check, pairs, n, 0.03, 0.0, seeds, members)
    rel = cr.relation(pairs, 0.03, 0.0)["rel"]
    expect = {"diagonal": "adj", "unmasked": "S", "pad_bits": "adj", "tie_high": "rank2", "seed_not_first": "lists", "rank_float32": "rank2",
              "ascending_S": "lists"}
    assert set(expect) == set(c2.WRONG)
    for wrong, stage in expect.items():
        M = c2.adjacency(rel, wrong)
        S, d2 = c2.second_order(M, wrong)
        if wrong in ("tie_high", "rank_float32"):               # integers with ties / beyond 2^24, where these variants differ
            d2 = (d2 // 8) * 8 + (1 << 25) * (wrong == "rank_float32") + (np.arange(P) % 2) * (wrong == "rank_float32")
            hr = np.empty(P, np.int32)
            check.c2_rank(d2.ctypes.data_as(cc.P_), P, hr.ctypes.data_as(cc.P_))
            assert np.array_equal(hr, c2.ranks2(d2)) and not np.array_equal(hr, c2.ranks2(d2, wrong)), wrong
            continue
        ref = dict(adj=c2.bits(M, n, wrong), degree_packed=M.sum(axis=1).astype(np.int32), S=S, degree2_packed=d2, rank2_packed=c2.ranks2(d2, wrong),
                   score2_packed=c2.score2_of(d2, dtype))
        lists = c2.member_lists(S, ref["rank2_packed"], seeds, members, wrong)
        assert stage in compare(h, ref, lists, n, P), wrong
    lst = h["lists"][0][h["lists"][0] >= 0]                     # the sums tell the order of the members
    scaled = (pairs * 2.0 ** np.random.default_rng(1).integers(-12, 13, (P, 1))).astype(dtype)
    sums, _ = cc.header_fit(check, scaled, h["lists"][:1])
    assert rc.same_bits(sums[0], c2.list_sums(scaled, lst)) and not rc.same_bits(sums[0], c2.list_sums(scaled, lst[::-1]))
    bad = h["poses"].copy()
    bad[:, :9] = bad[:, [0, 3, 6, 1, 4, 7, 2, 5, 8]]            # the transposed rotation is refused
    assert c2.poses_hold(h["poses"], pairs, h["lists"])[0] and not c2.poses_hold(bad, pairs, h["lists"])[0]


def test_designed_graphs(check):
    """a complete graph, an empty one, one clique plus isolated rows: exact duplicates are compatible at min_length 0 and not above it"""
    dtype = np.float64
    rng = np.random.default_rng(4)
    x = rng.uniform(0, 1, (40, 3))
    full = np.concatenate((x, x + 0.25), axis=1).astype(dtype)               # a pure translation: every pair compatible
    h = cc.header_stages(check, full, 40, 0.01, 0.0, 8, 5)
    assert (h["degree"] == 39).all() and (h["degree2"] == 39 * 38).all() and np.array_equal(h["rank2"], np.arange(40))
    assert np.array_equal(h["lists"][0], [0, 1, 2, 3, 4]) and np.array_equal(h["lists"][3], [3, 0, 1, 2, 4]) and (h["score2"] == 1).all()
    dup = np.tile(full[:1], (6, 1))                                          # exact duplicates
    assert (cc.header_stages(check, dup, 6, 0.01, 0.0, 2, 3)["degree"] == 5).all()
    h = cc.header_stages(check, dup, 6, 0.01, 1e-6, 2, 3)
    assert not h["adj"].any() and not h["degree2"].any() and (h["score2"] == 0).all()
    assert np.array_equal(h["lists"], [[0, -1, -1], [1, -1, -1]]) and np.array_equal(h["poses"], np.tile(rr.IDENTITY, (2, 1)))
    mixed = full.copy()
    mixed[10:, 3:] = rng.uniform(0, 50, (30, 3)) * np.arange(1, 31)[:, None]  # rows 10.. keep no length: a clique of 10 plus isolated rows
    h = cc.header_stages(check, mixed, 40, 0.01, 0.0, 12, 32)
    M = c2.adjacency(cr.relation(mixed, 0.01, 0.0)["rel"])
    assert M[:10, :10].sum() == 90 and M.sum() == 90
    assert (h["degree2"][:10] == 9 * 8).all() and not h["degree2"][10:].any()
    assert np.array_equal(h["lists"][2][:10], [2, 0, 1, 3, 4, 5, 6, 7, 8, 9]) and (h["lists"][2][10:] == -1).all()      # members > the candidates
    assert np.array_equal(h["lists"][10], [10] + [-1] * 31)


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype", DTYPES)
def test_second_order_separates_where_first_order_does_not(dtype):
    overlap = 0
    for seed in range(5):
        a = cr.recovery_case(seed, n=600, inliers=18, dtype=dtype)
        out = c2.consensus_ref(a["x"], a["y"], a["idx"], 0.05, seeds=32, members=10, refine=0)
        truth = a["truth"]
        d2, d1 = out["degree2"], out["degree"]
        print("seed %d %s: degree2 inliers min %d, outliers max %d; degree inliers min %d, outliers max %d; inliers found %d, rotation error %.2e"
              % (seed, np.dtype(dtype).name, d2[truth].min(), d2[~truth].max(), d1[truth].min(), d1[~truth].max(), int(out["inliers"][truth].sum()),
                 cr.rotation_angle(out["pose"][:9], a["C"])))
        assert d2[truth].min() > d2[~truth].max()
        top = np.zeros(600, dtype=bool)
        top[out["rows"][out["rank2_packed"] < 18]] = True
        assert np.array_equal(top, truth)
        overlap += d1[truth].min() <= d1[~truth].max()
        assert out["inliers"][truth].all()
        assert cr.rotation_angle(out["pose"][:9], a["C"]) < 5e-3
    assert overlap >= 1


# ------------------------------------------------------------------ 3
def _bad(fn, *a, **kw):
    with pytest.raises(ValueError):
        fn(*a, **kw)


def test_argument_checks_of_the_python_functions():
    x, y, idx = torch.zeros(5, 3), torch.zeros(7, 3), torch.zeros(5, dtype=torch.int64)
    for thr in (0, -1.0, float("inf"), float("nan"), "0.1", None, True):
        _bad(second_order_compatibility, x, y, idx, thr)
        _bad(consensus_correspondences, x, y, idx, thr)
    for L in (-1e-9, float("nan"), float("inf"), None, True):
        _bad(second_order_compatibility, x, y, idx, 0.1, min_length=L)
        _bad(consensus_correspondences, x, y, idx, 0.1, min_length=L)
    _bad(second_order_compatibility, x, y, idx, 0.1, return_adjacency=1)
    for order in (0, 3, None, True, 1.5, "2"):
        _bad(prune_correspondences, x, y, idx, 0.1, 3, order=order)
    for seeds in (0, -1, 65537, 1.0, None, True):
        _bad(consensus_correspondences, x, y, idx, 0.1, seeds=seeds)
    for members in (2, 33, 0, 4.0, None, True):
        _bad(consensus_correspondences, x, y, idx, 0.1, members=members)
    for refine in (-1, 9, 1.0, None, True):
        _bad(consensus_correspondences, x, y, idx, 0.1, refine=refine)
    for it in (0.0, -1.0, float("nan"), "x", True):
        _bad(consensus_correspondences, x, y, idx, 0.1, inlier_threshold=it)
    _bad(consensus_correspondences, x, y, idx, 0.1, return_hypothesis=1)
    _bad(consensus_correspondences, x, y, idx.float(), 0.1)
    _bad(second_order_compatibility, x, y, idx[:4], 0.1)
