"""CPU checks of dicp_amd.evaluate (evaluate_registration, information_matrix, best_pose) that need no GPU.

The rules of ``dicp_amd/csrc/dicp_evaluate.h`` -- the lines the HIP kernels run -- are compiled with g++ through
tests/hostcheck/evaluate_check.cpp, run in a serial loop over a host-built grid and held to the numpy restatement tests/evaluate_ref.py
bit for bit in both dtypes: idx, d2, counts, the ten sums, fitness and rmse.  The rows have very different magnitudes, so a restatement
that sums in ascending order is refused by the same comparison.  Designed inputs sit on every comparison of the definition, the
information matrix is held to an independent accumulation inside the bound tests/evaluate_cases.py derives, the scene's candidates rank
as the float64 brute force ranks them, and the argument checks of the Python functions run before any device work.
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.evaluate import best_pose, evaluate_registration, information_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import evaluate_cases as ec  # noqa: E402
import evaluate_ref as er  # noqa: E402

DTYPES = ec.DTYPES


@pytest.fixture(scope="module")
def check():
    return ec.build()


def test_constants(check):
    assert (check.ec_tile(), check.ec_terms(), check.ec_h_max()) == (er.TILE, er.TERMS, er.H_MAX)


# ------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", (1, 700))
@pytest.mark.parametrize("n", (1, 63, 65, 255, 257, 513, 1000))
def test_the_header_is_the_restatement(check, dtype, n, m):
    for H in (1, 3):
        x, y, T, radius = ec.magnitudes_case(n + m + H, n, m, H, dtype)
        got = ec.header_run(check, x, y, T, radius)
        ref = er.evaluate_ref(x, y, T, radius)
        assert ec.differences(got, ref) == []
        assert got["counts"][0] >= 0.9 * n and got["stats"][2] == m
        if n >= 63 and m > 1:                 # (against one target row every term but e is the same number: any order gives the same sum)
            assert "sums" in ec.differences(got, er.evaluate_ref(x, y, T, radius, wrong="ascending"))      # a sum in ascending order is refused
    if n >= 63 and m > 1:
        assert ec.differences(got, er.evaluate_ref(x, y, T, radius, wrong="unfused")) != []                 # ... and so is an unfused query


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_tile_tree(check, dtype):
    rng = np.random.default_rng(5)
    v = rng.standard_normal((er.TILE, 3)) * 2.0 ** rng.integers(-30, 30, (er.TILE, 1))
    tree = er.tile_tree(v)
    by_hand = v.copy()                                                    # the definition, written out: v_l + v_(l + off), off = 1 .. 128
    for off in (1, 2, 4, 8, 16, 32, 64, 128):
        for lo in range(0, er.TILE, 2 * off):
            by_hand[lo] = by_hand[lo] + by_hand[lo + off]
    assert ec.same_bits(tree, by_hand[0]) and not ec.same_bits(tree, er.sums_of(v, wrong="ascending"))
    assert ec.same_bits(er.sums_of(v[:200]), er.tile_tree(np.concatenate((v[:200], np.zeros((56, 3))))))   # rows at or past n contribute +0


# ------------------------------------------------------------------ designed inputs
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(ec.designed(np.float32)))
def test_designed_inputs(check, dtype, name):
    case = ec.designed(dtype)[name]
    ref = ec.ref_of(case)
    case["expect"](ref)
    got = ec.header_run(check, case["x"], case["y"], case["T"], case["radius"], case.get("x_rows"), case.get("y_rows"))
    assert ec.differences(got, ref) == []
    case["expect"](got)
    if "stats" in case:
        assert tuple(got["stats"][:2]) == case["stats"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_wrong_restatements_are_refused(check, dtype):
    cases = ec.designed(dtype)
    for name, wrong in (("duplicate", "tie_high"), ("on_the_radius", "strict")):
        case = cases[name]
        got = ec.header_run(check, case["x"], case["y"], case["T"], case["radius"])
        assert ec.differences(got, ec.ref_of(case)) == [] and "idx" in ec.differences(got, ec.ref_of(case, wrong=wrong))


# ------------------------------------------------------------------ the information matrix
@pytest.mark.parametrize("dtype", DTYPES)
def test_information_matrix_against_an_independent_accumulation(check, dtype):
    for seed, n, m in ((1, 257, 700), (2, 1000, 700), (3, 65, 1)):
        x, y, T, radius = ec.magnitudes_case(seed, n, m, 3, dtype)
        got = ec.header_run(check, x, y, T, radius)
        for h in range(3):
            L = er.assemble(got["sums"][h], got["counts"][h])
            plain, bound = ec.info_bound(y, got["idx"][h])
            assert np.all(np.abs(L - plain) <= bound), (seed, h, np.abs(L - plain).max())
            assert np.array_equal(L[3:, 3:], float(got["counts"][h]) * np.eye(3)) and np.array_equal(L, L.T)
            assert np.linalg.eigvalsh(L).min() >= -bound.sum()
        assert got["counts"][0] > 0 and np.abs(er.assemble(got["sums"][0], got["counts"][0])).max() > 0
    x, y, T, radius = ec.magnitudes_case(4, 70, 90, 2, dtype)
    none = ec.header_run(check, x, y, T, radius, y_rows=0)
    assert not er.assemble(none["sums"][0], none["counts"][0]).any()                  # an empty target: a zero matrix


# ------------------------------------------------------------------ the scene, on the restatement and on the g++ build
@pytest.mark.parametrize("dtype", DTYPES)
def test_scene_ranking(check, dtype):
    x, y, T = ec.scene_case(dtype)
    assert x.shape == (1275, 3)
    got = ec.header_run(check, x, y, T, ec.SCENE_DISTANCE)
    ref = er.evaluate_ref(x, y, T, ec.SCENE_DISTANCE)
    assert ec.differences(got, ref) == []
    for o in (got, ref):
        assert er.best_pose_ref(o["counts"], o["rmse"]) == 0 and o["fitness"][0] == 1.0 and o["fitness"][1] < 0.5 and o["fitness"][2] < 0.5
    for h in range(3):
        fit, rmse, count = ec.brute_force64(x, y, T[h], ec.SCENE_DISTANCE)
        assert abs(fit - ec.SCENE_FITNESS[h]) < 2e-3 and abs(rmse - ec.SCENE_RMSE[h]) < 1e-2 * ec.SCENE_RMSE[h]
        if h == 0:
            assert count == got["counts"][0] and abs(got["rmse"][0] - rmse) <= ec.rmse_bound(x, T[0], ec.SCENE_DISTANCE, dtype)


# ------------------------------------------------------------------ the Python front: ValueError before any device work
def _bad(f, *args, **kw):
    with pytest.raises(ValueError, match=f.__name__):
        f(*args, **kw)


def test_argument_checks():
    src, tgt, T = torch.zeros(5, 3), torch.zeros(7, 3), torch.eye(4)
    bs, bt, bT = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3), torch.eye(4).repeat(2, 3, 1, 1)
    for f in (evaluate_registration, information_matrix):
        for bad_T in (torch.eye(3), torch.zeros(4, 5), torch.zeros(4), torch.zeros(2, 3, 4, 4), torch.zeros(0, 4, 4), torch.eye(4).double(), torch.eye(4).half(),
                      torch.eye(4).long(), torch.eye(4).numpy(), None, [torch.eye(4)]):
            _bad(f, src, tgt, bad_T, 0.1)
        for bad_T in (torch.eye(4), torch.zeros(3, 4, 4), torch.zeros(3, 2, 4, 4), torch.zeros(2, 0, 4, 4), torch.zeros(2, 2, 2, 4, 4), torch.zeros(2, 3, 4, 4).double()):
            _bad(f, bs, bt, bad_T, 0.1)
        for r in (0, 0.0, -1.0, float("inf"), float("nan"), "0.1", None, True, torch.tensor([0.1]), torch.tensor(1), 1e-46, 1e39):
            _bad(f, src, tgt, T, r)
        _bad(f, [src], [tgt], T, 0.1)                                       # lists of clouds are not offered
        _bad(f, src, tgt.double(), T, 0.1)
        _bad(f, src.half(), tgt.half(), T.half(), 0.1)
        _bad(f, src[:, :2], tgt, T, 0.1)
        _bad(f, src, bt, T, 0.1)
        _bad(f, bs, bt[:1], bT, 0.1)
        _bad(f, src, tgt, T, 0.1, source_rows=torch.tensor([3]))            # row counts need a padded batch
        _bad(f, bs, bt, bT, 0.1, source_rows=torch.tensor([6, 1]))
        _bad(f, bs, bt, bT, 0.1, target_rows=torch.tensor([1.0, 2.0]))
        _bad(f, bs, bt, bT, 0.1, target_rows=torch.tensor([1, 2, 3]))
    _bad(evaluate_registration, torch.zeros(2, 300, 3), torch.zeros(2, 7, 3), torch.zeros(2, 65537, 4, 4), 0.1)            # H out of range
    big = torch.zeros(1, 3).expand(40000 * 256, 3)
    _bad(evaluate_registration, big, tgt, torch.zeros(1, 4, 4).expand(60000, 4, 4), 0.1)                                    # the launch grid does not fit
    for flag in (1, 0, None, "yes"):
        _bad(evaluate_registration, src, tgt, T, 0.1, return_correspondences=flag)


def test_best_pose_order():
    T = torch.arange(2 * 5 * 16, dtype=torch.float32).reshape(2, 5, 4, 4)
    counts = torch.tensor([[3, 9, 9, 9, 2], [0, 0, 0, 0, 0]], dtype=torch.int32)
    rmse = torch.tensor([[0.0, 0.5, 0.25, 0.25, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    best, Tb = best_pose(T, counts, rmse)
    assert best.dtype == torch.int64 and best.tolist() == [2, 0] and torch.equal(Tb, T[[0, 1], [2, 0]])       # count, then rmse, then the lowest h
    rng = np.random.default_rng(0)
    for _ in range(20):
        c = rng.integers(0, 4, (6, 7)).astype(np.int32)
        r = rng.integers(0, 3, (6, 7)).astype(np.float64) / 4
        best, Tb = best_pose(torch.zeros(6, 7, 4, 4), torch.from_numpy(c), torch.from_numpy(r))
        assert best.tolist() == [er.best_pose_ref(c[b], r[b]) for b in range(6)]
    b1, T1 = best_pose(T[0], counts[0], rmse[0])                                                              # the single-pair form
    assert b1.dim() == 0 and int(b1) == 2 and torch.equal(T1, T[0, 2])
    for args in ((T, counts[:, :4], rmse), (T, counts, rmse[0]), (T, counts.float(), rmse), (T, counts, counts), (T[0, 0], counts[0, 0], rmse[0, 0]),
                 (T[:, :0], counts[:, :0], rmse[:, :0]), (T.numpy(), counts, rmse)):
        _bad(best_pose, *args)
