"""CPU checks of correspondence_compatibility / prune_correspondences (dicp_amd/compat.py) that need no GPU.

The rules of ``dicp_amd/csrc/dicp_compat.h`` -- the lines the HIP kernels run -- are compiled with g++ through
tests/hostcheck/compat_check.cpp, run in a serial loop and held to the numpy restatement tests/compat_ref.py bit for bit in both dtypes:
A, B, e, the relation, the degree, w and v of every iteration, and the ranks.  The exact edges are designed tables whose results are
stated here; every deliberately wrong restatement is shown to be refused by the same comparisons; the decisions are held to a float64
evaluation inside the bound of tests/compat_cases.py; the recovery case of the GPU test is evaluated on the restatement alone; and the
argument checks of the two Python functions run before any device work.
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.match import correspondence_compatibility, prune_correspondences

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import compat_cases as cc  # noqa: E402
import compat_ref as cr  # noqa: E402
import match_ref as mr  # noqa: E402
import ransac_ref as rr  # noqa: E402

DTYPES = [np.float32, np.float64]
same_bits = cc.same_bits


@pytest.fixture(scope="module")
def check():
    return cc.build()


def tables(dtype):
    return cc.edge_tables(dtype) + [cc.few_pairs(dtype, P) for P in range(4)]


def test_fast_fma64_is_the_exact_one_on_the_chains():
    rng = np.random.default_rng(1)
    pts = rng.uniform(0, 10, (14, 3))
    s_fast, s_exact = np.zeros((14, 14)), np.zeros((14, 14))
    for a in range(3):
        t = pts[:, None, a] - pts[None, :, a]
        s_fast, s_exact = rr.fma64_fast(t, t, s_fast), mr.fma64(t, t, s_exact)
        assert same_bits(s_fast, s_exact)
    assert same_bits(cr.len2(pts), s_exact)
    assert not same_bits(s_exact, ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))       # separately rounded squares are refused


# ------------------------------------------------------------------ the host build, bit for bit
def held(check, pairs, thr, L, iterations):
    """every stage of the header on packed pairs against the restatement; -> the restatement's (relation dict, ws, vs, ranks)"""
    dt = pairs.dtype
    P = pairs.shape[0]
    ref = cr.relation(pairs, thr, L)
    A, B, e, rel = cc.header_relation(check, pairs, thr, L)
    assert same_bits(A, ref["A"]) and same_bits(B, ref["B"]) and same_bits(e, ref["e"])
    assert np.array_equal(rel, ref["rel"])
    assert np.array_equal(rel, rel.T)                           # symmetric bit for bit
    deg, w, v = cc.header_scores(check, pairs, iterations, thr, L)
    assert np.array_equal(deg, cr.degree_of(ref["rel"]))
    ws, vs = cr.power(ref["rel"], iterations, dt)
    for t in range(iterations):
        assert same_bits(w[t], ws[t]), t
        assert same_bits(v[t], vs[t]), t
    score = vs[-1] if vs else np.ones(P, dtype=dt)
    rk = cr.ranks(score)
    assert np.array_equal(cc.header_rank(check, score), rk)
    assert sorted(rk.tolist()) == list(range(P))                # a permutation
    if iterations and P and P < (1 << 24):
        assert np.array_equal(ws[0], (deg + 1).astype(dt))      # w^1 = degree + 1 exactly
        assert all(float(x.max()) >= 1.0 for x in ws) and all(float(x.max()) == 1.0 for x in vs)
    return ref, ws, vs, rk


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,L", ((1, 0.0), (2, 0.0), (3, 0.5), (40, 0.0), (131, 2.0)))
def test_host_build_matches_restatement(check, dtype, P, L):
    rng = np.random.default_rng(P)
    x, y, idx = cc.cloud(rng, P + 9, P + 30, P, dtype, rows=P + 5)
    rows, pairs = rr.packed(x, y, idx, P + 5)
    assert rows.size == P
    ref, ws, vs, rk = held(check, pairs, cc.TAU, L, 10)
    if P >= 40:
        assert 0 < cr.degree_of(ref["rel"]).max() < P - 1       # neither empty nor full
        assert len(np.unique(vs[-1])) > P // 4


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_edges(check, dtype):
    T = dtype
    got = {}
    for tb in tables(dtype):
        rows, pairs = rr.packed(tb["x"], tb["y"], tb["idx"])
        ref, ws, vs, rk = held(check, pairs, tb["threshold"], tb["min_length"], 4)
        got[tb["name"]] = dict(ref, rows=rows, deg=cr.degree_of(ref["rel"]), score=vs[-1] if rows.size else np.ones(0, T), rank=rk)
    g = got["lattice"]
    assert list(g["a"][0]) == [0, 5, 13, 5, 10] and list(g["b"][0]) == [0, 4, 12, 7, 10] and list(g["e"][0]) == [0, 1, 1, -2, 0]
    assert list(g["rel"][0]) == [True, True, True, False, True]                 # |e| == thr is in, 2 is out
    g = got["one_ulp"]
    one = T(1)
    assert g["e"][0, 1] == np.nextafter(one, T(2)) and g["e"][0, 2] == one and g["e"][0, 3] == np.nextafter(one, T(0))
    assert list(g["rel"][0, 1:]) == [False, True, True] and list(g["rel"][1:, 0]) == [False, True, True]
    assert got["length_on_L"]["deg"].tolist() == [1, 1] and got["length_below_L"]["deg"].tolist() == [0, 0] and got["b_below_L"]["deg"].tolist() == [0, 0]
    g = got["duplicates"]
    assert g["A"][0, 1] == 0 and g["B"][0, 2] == 0 and g["e"][0, 1] == T(-0.03125) and g["e"][0, 2] == T(0.03125)
    assert g["deg"].tolist() == [3, 3, 3, 3]
    assert got["duplicates_min_length"]["deg"].tolist() == [1, 2, 2, 3]        # a zero length vouches for nobody; rule 2 on the diagonal too:
    assert not got["duplicates_min_length"]["rel"].diagonal().any() and got["duplicates"]["rel"].diagonal().all()   # the self term is rule 4's, not rule 2's
    g = got["shared_target"]
    assert g["B"][0, 1] == 0 and g["rel"][0, 1] and g["deg"].tolist() == [3, 3, 3, 3]
    g = got["shared_target_min_length"]                         # two matches on one target point stop vouching for each other
    assert not g["rel"][0, 1] and g["deg"].tolist() == [2, 2, 3, 3]
    g = got["not_live"]
    assert g["rows"].tolist() == [0, 2, 4] and g["deg"].tolist() == [2, 2, 2]
    g = got["all_tied"]
    assert g["deg"].tolist() == [8] * 9 and np.all(g["score"] == 1) and g["rank"].tolist() == list(range(9))
    g = got["two_cliques"]
    assert g["deg"].tolist() == [4] * 10 and np.all(g["score"] == 1) and g["rank"].tolist() == list(range(10))
    assert not g["rel"][0::2, 1::2].any()
    for P in range(4):
        g = got["P%d" % P]
        assert g["rows"].tolist() == sorted([5, 1, 3][:P]) and g["deg"].tolist() == [max(P - 1, 0)] * P and np.all(g["score"] == 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_front_of_the_restatement_on_the_tables(dtype):
    """compat_ref's scatter to the original rows, the zeros on rows that are not live, keep at and past P"""
    tb = [t for t in cc.edge_tables(dtype) if t["name"] == "not_live"][0]
    out = cr.compat_ref(tb["x"], tb["y"], tb["idx"], tb["threshold"], 3, keep=2)
    assert out["degree"].tolist() == [2, 0, 2, 0, 2, 0] and out["score"].tolist() == [1, 0, 1, 0, 1, 0]
    assert out["idx_kept"].tolist() == [0, -1, 2, -1, -1, -1] and out["idx_kept"].dtype == np.int64
    for keep in (3, 4, 100):
        assert cr.compat_ref(tb["x"], tb["y"], tb["idx"], tb["threshold"], 3, keep=keep)["idx_kept"].tolist() == [0, -1, 2, -1, 4, -1]
    i32 = cr.compat_ref(tb["x"], tb["y"], tb["idx"].astype(np.int32), tb["threshold"], 0, keep=1)
    assert i32["idx_kept"].dtype == np.int32 and i32["idx_kept"].tolist() == [0, -1, -1, -1, -1, -1] and i32["score"].tolist() == [1, 0, 1, 0, 1, 0]
    big = tb["idx"].copy()
    big[2] = 11                                                 # at or past m: clamped to the last row, whose y is finite
    assert cr.compat_ref(tb["x"], tb["y"], big, tb["threshold"], 1)["P"] == 3
    assert cr.compat_ref(tb["x"], tb["y"], tb["idx"], tb["threshold"], 1, x_rows=3)["rows"].tolist() == [0, 2]


# ------------------------------------------------------------------ wrong variants
def test_wrong_variants_are_refused(check):
    for dtype in DTYPES:
        rng = np.random.default_rng(23)
        x, y, idx = cc.cloud(rng, 150, 200, 150, dtype, clamp=False)
        _, pairs = rr.packed(x, y, idx)
        thr = cc.TAU
        deg, w, v = cc.header_scores(check, pairs, 6, thr)
        rel = cr.relation(pairs, thr)["rel"]

        def agrees(wrong, rel_w=None):
            ws, vs = cr.power(rel if rel_w is None else rel_w, 6, dtype, wrong)
            return all(same_bits(w[t], ws[t]) and same_bits(v[t], vs[t]) for t in range(6))
        assert agrees(None)
        for wrong in ("no_self", "descending", "pairwise", "sum_norm"):
            assert not agrees(wrong), wrong
        assert not np.array_equal(deg, cr.degree_of(cr.relation(pairs, thr, wrong="squared")["rel"]))
        # `<` for `<=`: the lattice table has pairs exactly on the threshold
        tb = cc.edge_tables(dtype)[0]
        _, lp = rr.packed(tb["x"], tb["y"], tb["idx"])
        ldeg = cc.header_scores(check, lp, 1, tb["threshold"])[0]
        assert np.array_equal(ldeg, cr.degree_of(cr.relation(lp, tb["threshold"])["rel"]))
        assert not np.array_equal(ldeg, cr.degree_of(cr.relation(lp, tb["threshold"], wrong="strict_less")["rel"]))
        # rank ties to the higher index: scores with ties
        score = np.round(v[-1] * 8).astype(dtype) / dtype(8)
        rk = cc.header_rank(check, score)
        assert len(np.unique(score)) < score.size
        assert np.array_equal(rk, cr.ranks(score)) and not np.array_equal(rk, cr.ranks(score, wrong="tie_high"))


# ------------------------------------------------------------------ decisions against float64
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", (0, 1))
def test_decisions_against_float64(check, dtype, seed):
    rng = np.random.default_rng(40 + seed)
    x, y, idx = cc.cloud(rng, 300, 400, 300, dtype, inlier_ratio=0.5, clamp=False)
    _, pairs = rr.packed(x, y, idx)
    thr = 0.046875 if seed else cc.TAU                          # 3 / 64: exactly representable; 0.05 is rounded to T
    rel = cc.header_relation(check, pairs, thr)[3]
    rel64, margin, bound = cr.relation64(pairs, float(dtype(thr)))
    off = ~np.eye(300, dtype=bool)
    ok = (margin > bound) & off
    share = ok.sum() / off.sum()
    print("%s: %.5f of the pairs qualify, largest bound / tau %.3g, compatible %d" % (np.dtype(dtype).name, share, bound.max() / thr, rel64[off].sum()))
    assert share >= cc.MIN_QUALIFY                              # a condition on the inputs
    assert rel64[off].sum() > 1000
    assert np.array_equal(rel[ok], rel64[ok])
    assert not np.array_equal(cr.relation(pairs, thr, wrong="squared")["rel"][ok], rel64[ok])


# ------------------------------------------------------------------ the recovery case, on the restatement alone
def recovered(a, seed, dtype):
    """rules 1-5 and then ransac_ref on the kept set -> (compat_ref's dict, ransac_ref's dict on the kept set, on every match)"""
    out = cr.compat_ref(a["x"], a["y"], a["idx"], cc.TAU, 10, keep=60)
    kw = dict(hypotheses=64, seed=cc.RANSAC_SEED, refine=1)
    return out, rr.ransac_ref(a["x"], a["y"], out["idx_kept"], 3 * cc.TAU, **kw), rr.ransac_ref(a["x"], a["y"], a["idx"], 3 * cc.TAU, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", range(5))
def test_recovery_on_the_restatement(dtype, seed):
    a = cr.recovery_case(seed, dtype=dtype)
    truth = a["truth"]
    out, pruned, plain = recovered(a, seed, dtype)
    deg, kept = out["degree"], out["kept"]
    assert deg[truth].min() > deg[~truth].max()                 # the degrees alone separate the two sets
    assert kept.sum() == 60 and (kept & truth).sum() >= 0.95 * 60
    err = cr.rotation_angle(pruned["pose"][:9], a["C"])
    print("case %d %s: inlier degrees >= %d, outlier degrees <= %d, %d of 60 kept are true; H = 64: pruned %d inliers, %.3g rad; unpruned %d inliers"
          % (seed, np.dtype(dtype).name, deg[truth].min(), deg[~truth].max(), (kept & truth).sum(), pruned["inliers"].sum(), err, plain["inliers"].sum()))
    assert err < 0.01
    assert pruned["inliers"][kept & truth].all()                # every true kept pair within 3 x threshold (RANSAC's own)
    assert plain["inliers"].sum() < truth.sum()                 # the same H and seed on every match do not find the motion


# ------------------------------------------------------------------ the Python fronts: ValueError before any device work
def _bad(fn, *args, **kw):
    with pytest.raises(ValueError):
        fn(*args, **kw)


def test_argument_checks_of_the_python_functions():
    x, y, idx = torch.zeros(5, 3), torch.zeros(7, 3), torch.zeros(5, dtype=torch.int64)
    fns = ((correspondence_compatibility, ()), (prune_correspondences, (3,)))
    for fn, keep in fns:
        for thr in (0, 0.0, -1.0, float("inf"), float("nan"), "0.1", None, True, torch.tensor(0.1)):
            _bad(fn, x, y, idx, thr, *keep)
        for L in (-1e-9, -1, float("inf"), float("nan"), "0", None, True, torch.tensor(0.0)):
            _bad(fn, x, y, idx, 0.1, *keep, min_length=L)
        for it in (-1, 65, 10.0, True, None, "3"):
            _bad(fn, x, y, idx, 0.1, *keep, iterations=it)
        # the forms and checks of align_correspondences
        _bad(fn, x, y, idx.float(), 0.1, *keep)
        _bad(fn, x, y, idx[:4], 0.1, *keep)
        _bad(fn, x, y, idx + 7, 0.1, *keep)
        _bad(fn, x[:, :2], y, idx, 0.1, *keep)
        _bad(fn, [x], [y], idx, 0.1, *keep)
        _bad(fn, x, y, idx, 0.1, *keep, x_rows=torch.tensor([3]))
        _bad(fn, x[None], y[None], idx[None], 0.1, *keep, x_rows=torch.tensor([6]))
        _bad(fn, x.half(), y.half(), idx, 0.1, *keep)
        _bad(fn, x, y.double(), idx, 0.1, *keep)
    for keep in (0, -1, 2.0, True, None, "3", torch.tensor(3)):
        _bad(prune_correspondences, x, y, idx, 0.1, keep)
    with pytest.raises(TypeError):
        prune_correspondences(x, y, idx, 0.1)                   # keep has no default
