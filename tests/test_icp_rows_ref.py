"""The inputs of tests/test_gpu_icp_rows.py, judged on the float64 reference alone (CPU, no GPU, no library): properties of the INPUTS that the GPU
comparison's bars rest on.  Where a cloud misses one, its rows are drawn differently in tests/icp_rows_ref.py -- no bar here is loosened."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_rows_ref as R  # noqa: E402

from dicp_amd.synthetic import make_pairs  # noqa: E402
from oracle import dicp_oracle as O  # noqa: E402

TOL_CASES = [k for k, c in R.CASES.items() if c.mode == "tol"]


def test_the_batch_holds_what_it_says():
    d = R.batch()
    assert d["source"].shape == (R.N, R.N_PAD, 3) and d["target"].shape == (R.N, R.M_PAD, 6) and max(R.LS) == R.N_PAD and max(R.LT) == R.M_PAD
    for b in range(R.N):
        n, m = R.LS[b], R.LT[b]
        s, t = make_pairs(1, n, m, seed=R.SEED, dtype=torch.float64, first=b)
        assert torch.equal(d["source"][b, :n], s[0]) and torch.equal(d["target"][b, :m], t[0])
        assert bool(torch.isfinite(d["w_point"][b, :n]).all()) and bool(torch.isfinite(d["T_init"][b]).all())
        sp, tp, wp = d["source"][b, n:], d["target"][b, m:], d["w_point"][b, n:]
        assert (n == R.N_PAD) == (R.SRC_PAD[b] == "none") == (R.W_PAD[b] == "none") and (m == R.M_PAD) == (R.TGT_PAD[b] == "none")
        if R.SRC_PAD[b] in ("nan", "big"):
            assert bool(torch.isnan(sp).all() if R.SRC_PAD[b] == "nan" else (sp == 1e30).all())
        if R.SRC_PAD[b] == "copy":
            assert torch.equal(sp[:min(n, len(sp))], s[0][:min(n, len(sp))])
        if R.TGT_PAD[b] == "nan":
            assert bool(torch.isnan(tp).all())
        if R.W_PAD[b] != "none":
            assert bool(torch.isnan(wp).all() if R.W_PAD[b] == "nan" else (wp == 1.0).all())
        # the per-point weights: zeros, and values on both sides of 0.3 at least 0.05 clear of it
        w = d["w_point"][b, :n]
        assert bool((w == 0).any()) and bool(((w > 0) & (w < 0.3)).any()) and bool((w > 0.3).any()) and float((w[w != 0] - 0.3).abs().min()) >= 0.05 - 1e-12
    wc = d["w_cloud"][:, 0]
    assert bool((wc < 0.3).any()) and bool((wc > 0.3).any()) and float((wc - 0.3).abs().min()) >= 0.05 - 1e-12
    for kind in ("nan", "big", "copy"):
        assert kind in R.SRC_PAD
    assert "moved" in R.TGT_PAD and "nan" in R.TGT_PAD and "one" in R.W_PAD and "nan" in R.W_PAD


def test_a_moved_target_pad_would_win_the_argmin_if_it_were_scored():
    """true_pose restates make_pairs' draws: the source under it lies within the noise of its own target rows (6 sigma per axis) -- and, for a cloud the
    reference has aligned, a pad row built from it is nearer to its source point than the real match, for nearly every row."""
    d = R.batch()
    ref = R.reference("pl-diff-3-huber-trim-const-t0-none")
    seen = 0
    for b in range(R.N):
        n, m = R.LS[b], R.LT[b]
        C, r = R.true_pose(b)
        moved = d["source"][b, :n] @ C.T + r
        dist = torch.cdist(moved, d["target"][b, :m, :3]).min(dim=1).values
        assert float(dist.max()) <= 6 * 0.01 * 3 ** 0.5, b
        if R.TGT_PAD[b] == "moved":
            assert ref[b]["converged"]
            pads = d["target"][b, m:, :3]
            assert torch.equal(pads[:min(n, len(pads))], moved[:min(n, len(pads))])
            k = min(n, len(pads))
            real = torch.cdist(ref[b]["pc"][:k], d["target"][b, :m, :3]).min(dim=1).values
            pad = torch.cdist(ref[b]["pc"][:k], pads).min(dim=1).values
            assert float((pad < real).double().mean()) > 0.9, b
            seen += 1
    assert seen >= 3


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_normal_matrix_is_well_conditioned(name):
    """cond(A) <= 1e6 at every iteration of every cloud: the rounding of a float64 solve then stays inside the 1e-10 bar of the pose."""
    for b, r in enumerate(R.reference(name)):
        assert float(r["cond"].max()) <= 1e6, (name, b, float(r["cond"].max()))
        assert r["deltas"].shape[0] == r["costs"].shape[0] == r["weights"].shape[0] == int(r["iterations"]) == len(r["cond"])
        for key in ("T", "pc", "deltas", "costs", "weights", "grad_source", "grad_target", "grad_T_init"):
            assert bool(torch.isfinite(r[key]).all()), (name, b, key)


@pytest.mark.parametrize("name", list(R.CASES))
def test_a_float32_solve_stays_inside_the_pose_bar(name):
    """The float32 bar of the pose is 1e-4.  A solve of A delta = b in float32 is off by at most cond(A) 2^-24 |delta| to first order, and what one
    iteration is off by the next ones carry on at worst: the sum over a cloud's iterations stays inside the bar (a cloud that wanders for all its
    iterations on 33 rows -- the one that must never converge -- comes nearest: 8e-5)."""
    for b, r in enumerate(R.reference(name)):
        assert float((r["cond"] * r["steps"]).sum()) * 2.0 ** -24 <= 1e-4, (name, b)


@pytest.mark.parametrize("name", list(R.CASES))
def test_no_step_is_near_the_tolerance_and_the_clouds_stop_early_late_and_never(name):
    """Every recorded step norm is a factor 2 away from the tolerance, above or below: a run in another precision stops at the same iteration (tolerance
    mode) and reports the same "converged" (both modes).  In tolerance mode the batch has a cloud that converges early, one that converges late and
    one that never does."""
    c = R.CASES[name]
    ref = R.reference(name)
    for b, r in enumerate(ref):
        s = r["steps"]
        assert bool(((s >= 2 * c.tol) | (s <= c.tol / 2)).all()), (name, b, s.tolist())
        assert r["converged"] == bool((s < c.tol).any()) and int(r["iterations"]) == len(s)
        assert c.mode == "const" or bool((s[:-1] >= c.tol).all())
    its = [int(r["iterations"]) for r in ref]
    conv = [r["converged"] for r in ref]
    assert any(conv) and max(its) == c.K
    if c.mode == "tol":
        assert not all(conv) and any(k and i <= 2 for k, i in zip(conv, its)) and any(k and i >= 4 for k, i in zip(conv, its)), (its, conv)


def test_float32_comparisons_keep_most_clouds():
    """tests/test_gpu_parity.py's cap on the margin rule, counted as that file counts it (over the scenarios one float32 test walks through): the clouds
    held to the float32 bars are at least 5x those left out.  Those left out, with the decision they pass within 1e-4 of: the planar (dim = 2) cases
    have near-ties of the argmin -- 3-D clouds flattened -- and two clouds carry a weight within rounding of the count threshold."""
    held = {name: R.float32_held(name) for name in R.CASES}
    out = sorted((name, int(b)) for name, h in held.items() for b in np.nonzero(~h)[0])
    assert sum(int(h.sum()) for h in held.values()) >= 5 * len(out), out
    assert out == [("pl-diff-3-huber-trim-const-t0-none", 7), ("pl-hard-2-huber-trim-const-t0.3-point", 2), ("pl-hard-2-huber-trim-const-t0.3-point", 3),
                   ("pt-diff-2-cauchy-trim-const-t0.3-none", 3), ("pt-diff-2-cauchy-trim-const-t0.3-none", 4)], [(o, R.reference(o[0])[o[1]]["margins"]) for o in out]
    for h in held.values():
        assert int(h.sum()) >= 6


@pytest.mark.parametrize("name", [k for k, c in R.CASES.items() if c.weight != "cloud"])
def test_the_reference_itself_is_indifferent_to_the_pads(name):
    """The oracle on the batch as the REFERENCE pads it (zero source rows of weight 0, the far target point) gives the per-cloud results: what the row
    counts promise is what the reference computes for a list.  (Not for an (N,1) weight: the reference cannot give a ragged batch one -- its zero
    rows would carry it.)"""
    c = R.CASES[name]
    src, tgt, w = R.reference_padding(c)
    out = O.icp_batched(src, tgt, R.batch()["T_init"], w, **R.oracle_kw(c))
    rows = 3 if c.icp_type == "pt2pt" else 1
    for b, r in enumerate(R.reference(name)):
        n, k = R.LS[b], int(r["iterations"])
        np.testing.assert_allclose(out["T"][b], r["T"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(out["pc"][b, :n], r["pc"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(out["deltas"][b, :k], r["deltas"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(out["costs"][b, :k], r["costs"], rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(out["weights"][b, :k, :n * rows], r["weights"], rtol=0, atol=1e-9)
        assert float(out["weights"][b, :, n * rows:].abs().sum()) == 0.0
        assert bool(out["stats"]["converged"][b]) == r["converged"] and float(out["stats"]["iterations"][b]) == r["iterations"]
        np.testing.assert_allclose(float(out["stats"]["matched_ratio"][b]), r["matched_ratio"], rtol=0, atol=1e-7)


def test_a_per_cloud_weight_reports_the_matched_count():
    """ICP.py:248,269 on a one-column weight: the ratio's denominator is 1 (or the weight is under the threshold and nothing counts)."""
    name = "pl-diff-3-cauchy-trim-const-t0.3-cloud"
    wc = R.batch()["w_cloud"][:, 0]
    for b, r in enumerate(R.reference(name)):
        assert r["matched_ratio"] == float(round(r["matched_ratio"])) and 0 <= r["matched_ratio"] <= R.LS[b]
        assert (r["matched_ratio"] == 0) == bool(wc[b] <= 0.3) or r["matched_ratio"] == 0
    assert R.reference(name)[5]["matched_ratio"] == 65.0
