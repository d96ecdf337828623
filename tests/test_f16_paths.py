"""The constructions and the model of tests/f16_paths.py, proved on the CPU before any GPU time is spent (no GPU needed).

For every case: each intermediate of score() rounds to itself, every query's class is certain (the one grey case apart), the predicted counters reach the
branch the case is named after (its `reach` predicates), and -- run with -s -- one line per case with the prediction.  Then the comparator the GPU tests
use is shown to see a wrong branch: the model with one rule mutated, fed through it as if it were a kernel's result, is refused.
tests/test_gpu_f16_paths.py holds the kernels to the same predictions."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f16_paths as P      # noqa: E402

CASES = P.cases()
SIZE_CASES = [c for m in P.SIZES_M for c in P.size_cases(m)]
BY_NAME = {c.name: c for c in CASES}


def _check(case):
    lines = []
    for form in ("brute", "sweep"):
        pred = P.predict(case, form)
        assert pred["exact"], "an intermediate of score() (or of the pose) is not a float32 number"
        assert (pred["grey"] > 0) == case.grey, "%d queries whose class is not certain" % pred["grey"]
        assert pred["ratio"] > 1.0
        if form in case.reach:
            assert case.reach[form](pred), "%s: the prediction does not reach '%s': %s" % (form, case.branch, P.describe(pred))
        lines.append("%-6s %s (smallest clear ratio %.2f)%s" % (form, P.describe(pred), pred["ratio"], "" if form in case.reach else "  [branch not named for this form]"))
    return lines


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_is_exact_certain_and_reaches_its_branch(case):
    assert case.reach, "a case names the branch it is there for"
    print("\n%s\n  branch: %s" % (case.name, case.branch))
    for line in _check(case):
        print("  " + line)


@pytest.mark.parametrize("m", P.SIZES_M)
def test_size_cases_are_exact_and_all_clear(m):
    for case in P.size_cases(m):
        for line in _check(case):
            pass
    print("\nsizes m=%d, n in 1..513: %s" % (m, line))


def test_the_starting_cloud_has_the_margins_the_model_needs():
    """Lattice 8 Z^3 in [-64, 64]^3, queries at most 0.5 per axis off a target: the runner-up is 0.5 (7.5^2 - 0.5^2) = 28 further at least, the clear
    rule asks for at most 2^-8 (0.375 + 1.5 * 64.5^2) = 24.4; the scale kernel picks s = 16 for an extent of 64."""
    rng = np.random.default_rng(0)
    y = P.pool(rng, 4096)
    assert P.scale_model(y)["s"] == 16.0 and P.scale_model(y)["nfar"] == 0
    pred = P.predict(P.Case("start", y, P.near(rng, y, 1300), "-"), "brute")
    assert pred["exact"] and pred["grey"] == 0 and pred["again"] == 0 and pred["scan"] == 0
    assert 1.14 < pred["ratio"] < 28 / 0.5


def test_scale_rule_edges():
    far = P.far_points(70)
    base = P.pool(np.random.default_rng(1), 4200, xmax=48.0)
    for k, m, use in ((64, 4096, True), (64, 4095, False), (65, 4160, False), (1, 64, True), (1, 63, False), (2, 128, True), (3, 128, False)):
        y = np.concatenate((far[:k], base[:m - k]))
        sm = P.scale_model(y)
        assert (sm["use_far"], sm["nfar"], sm["s"]) == (use, k if use else 0, 16.0 if use else 0.5), (k, m, sm)
    y = np.concatenate((base[:100], np.repeat(P.FAR0[None], 300, 0)))
    sm = P.scale_model(y)
    assert sm["cnt"] == 1 and sm["far"] == frozenset([100]) and int(sm["image"].sum()) == 100      # (the copies stay out of the image too)
    y = np.zeros((128, 3)); y[5] = P.FAR0
    assert not P.scale_model(y)["use_far"] and P.scale_model(y)["M2"] == 0.0
    y = np.full((10, 3), np.nan); y[3] = 1e30
    sm = P.scale_model(y)
    assert sm["s"] == 1.0 and not sm["finite"].any() and not sm["image"].any()


# ---------------------------------------------------------------- the comparator refuses a wrong branch
def _refused(case, form, mut, match):
    pred = P.predict(case, form)
    P.compare(P.as_result(pred), pred, "unmutated")          # the true model is accepted
    wrong = P.predict(case, form, mut=mut)
    with pytest.raises(AssertionError, match=match):
        P.compare(P.as_result(wrong), pred, "mutated")


@pytest.mark.parametrize("name,form", [("copies in three pieces, lowest index in half 0", "brute"), ("copies in two pieces that the wrong half would call three", "brute")])
def test_comparator_refuses_pieces_with_the_wrong_half(name, form):
    _refused(BY_NAME[name], form, P.MUTATIONS["pieces computed with the wrong half"], "AGAIN, SCAN")


@pytest.mark.parametrize("which", ["F16_SCAN_MAX taken as 5", "F16_SCAN_MAX taken as 7"])
def test_comparator_refuses_another_scan_threshold(which):
    case = BY_NAME["unsure queries per wave 1, 6, 7, 32"]
    _refused(case, "sweep", P.MUTATIONS[which], "AGAIN, SCAN")
    assert P.predict(case, "brute", mut=P.MUTATIONS[which])["again"] == P.predict(case, "brute")["again"]      # (the all-pairs form has no such switch)


def test_comparator_refuses_far_rows_only_below_64():
    for form in ("brute", "sweep"):
        _refused(BY_NAME["64 distinct far rows"], form, P.MUTATIONS["use_far with cnt < 64"], "scale")


@pytest.mark.parametrize("k", [3, 6])
@pytest.mark.parametrize("where", ["a middle", "last"])
def test_comparator_refuses_ties_by_sorted_position(k, where):
    case = BY_NAME["mirror ties in %d pieces, lowest index in the %s piece of the sorted order" % (k, where)]
    _refused(case, "sweep", P.MUTATIONS["tie rule by sorted position"], "indices differ")
    first = BY_NAME["mirror ties in %d pieces, lowest index in the first piece of the sorted order" % k]
    a, b = P.predict(first, "sweep"), P.predict(first, "sweep", mut=P.MUTATIONS["tie rule by sorted position"])
    assert np.array_equal(a["idx"], b["idx"])                 # (why both index orders are there: this one cannot tell the two rules apart)
    _refused(BY_NAME["two equal scores side by side in one run, sorted order the reverse of the original"], "sweep", P.MUTATIONS["tie rule by sorted position"], "indices differ")


def test_comparator_refuses_one_wrong_index_and_a_lost_far_row():
    case = BY_NAME["m = 128 with 2 far rows, one at index 0"]
    pred = P.predict(case, "brute")
    got = P.as_result(pred)
    got["idx"] = pred["idx"].copy(); got["idx"][0, 4] = 50    # the tie between the far row at index 0 and the image row at 50, answered with the image row
    with pytest.raises(AssertionError, match="indices differ"):
        P.compare(got, pred)
    got = P.as_result(pred); got["far"] = [frozenset([0])]
    with pytest.raises(AssertionError, match="far rows"):
        P.compare(got, pred)
