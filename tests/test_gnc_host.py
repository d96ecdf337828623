"""CPU checks of gnc_correspondences (dicp_amd/register.py) that need no GPU.

The rules of ``dicp_amd/csrc/dicp_gnc.h`` -- the lines the HIP kernel runs -- are compiled with g++ through
tests/hostcheck/gnc_check.cpp, run in a serial loop and held to the numpy restatement tests/gnc_ref.py: given each round's pose from the
trace, the residuals, the weights, the band counts, the mu sequence and the 18 sums (the tree included) bit for bit in both dtypes; the
restatement's own float64 SVD-Kabsch on a round's weights agrees with the round's pose inside the bound of tests/gnc_cases.py.  Designed
inputs sit on every comparison of the definition, every deliberately wrong restatement is shown to be refused by the same comparisons, the
recovery cases are evaluated on the g++ build, and the argument checks of the Python function run before any device work.

The composition for the hard ratios -- compat_ref.recovery_case(seed, inliers=60): 600 matches of which 60 are right, where GNC alone
loses seeds 1 and 3 (profiles/r32_gnc_edges.txt) -- is prune_correspondences(order=2, keep=60) at threshold 0.05, then
gnc_correspondences at threshold 0.05; it needs the pruning kernels and is asserted on the GPU (tests/test_gpu_gnc.py).
"""
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.match import gnc_correspondences

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gnc_cases as gc  # noqa: E402
import gnc_ref as gr  # noqa: E402
import ransac_ref as rr  # noqa: E402

DTYPES = gc.DTYPES
same_bits = gc.same_bits
POSE = slice(2 + gr.NKAB, gr.TRACE)
SUMS = slice(2, 2 + gr.NKAB)
EYE = np.array(gr.IDENTITY, dtype=np.float64)


@pytest.fixture(scope="module")
def check():
    return gc.build()


def test_constants(check):
    assert (check.gc_slots(), check.gc_iter_max(), check.gc_trace()) == (gr.SLOTS, gr.ITER_MAX, gr.TRACE)


def against_restatement(h, pairs, u, loss, thr, growth=1.4, iterations=128, wrong=None, bound=True):
    """is the g++ build's run (header_fit with detail) the restatement's, bit for bit, given each round's pose from the trace?"""
    ref = gr.gnc_ref(pairs, u, loss, thr, growth, iterations, wrong=wrong, poses=h["trace"][:, POSE])
    ok = (ref["rounds"], ref["status"]) == (h["rounds"], h["status"]) and same_bits(np.float64(ref["mu"]), np.float64(h["mu"]))
    ok = ok and same_bits(ref["weights"].astype(pairs.dtype), h["weights"])
    for k, r in enumerate(ref["records"][:h["rounds"] + 1]):
        ok = ok and same_bits(r["sums"], h["trace"][k, SUMS]) and same_bits(np.float64(r["mu"]), h["trace"][k, 0]) and r["band"] == h["trace"][k, 1]
        if k:
            ok = ok and same_bits(r["d"], h["d"][k]) and same_bits(r["w"], h["w"][k])
        if bound and ok and wrong is None:
            hold, wc, wr = gc.pose_holds(h["trace"][k, POSE], pairs, r["omega"])
            assert hold, (k, wc, wr)
    if h["rounds"] or pairs.shape[0] >= 3:
        ok = ok and same_bits(h["pose_last"], h["trace"][h["rounds"], POSE].astype(pairs.dtype))
    return bool(ok)


# ------------------------------------------------------------------ per round, bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("loss", (gr.TLS, gr.GM))
@pytest.mark.parametrize("P", (3, 4, 63, 65, 1023, 1025, 2049))
def test_rounds_match_the_restatement(check, dtype, loss, P):
    rng = np.random.default_rng(P + loss)
    pairs = gc.noisy_cloud(rng, P, dtype)
    pairs = (pairs * 2.0 ** rng.integers(-3, 4, (P, 1))).astype(dtype) if P > 4 else pairs     # rows of different sizes: the order of the sums shows
    for u in (None, rng.uniform(0.5, 1.5, P).astype(dtype)):
        h = gc.header_fit(check, pairs, u, loss, 0.04, detail=True)
        assert against_restatement(h, pairs, u, loss, 0.04)
        assert h["status"] in (gr.CONVERGED, gr.GUARDED) and h["rounds"] <= 128
        if P >= 63:
            assert not against_restatement(h, pairs, u, loss, 0.04, wrong="ascending")           # a sum in ascending order is refused


# ------------------------------------------------------------------ designed inputs
@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_chain(check, dtype):
    rng = np.random.default_rng(1)
    pairs = (rng.standard_normal((300, 6)) * 2.0 ** rng.integers(-20, 20, (300, 1))).astype(dtype)
    pose = rng.standard_normal(12)
    f = getattr(check, "gc_residual_" + gc.SFX[dtype])
    got = np.array([f(gc._ptr(pose), gc._ptr(np.ascontiguousarray(r))) for r in pairs])
    assert same_bits(got, gr.residual(pose, pairs))
    bad = pairs[:3].copy()
    bad[0, 1], bad[1, 4], bad[2, 0] = np.nan, np.inf, -np.inf
    assert [f(gc._ptr(pose), gc._ptr(np.ascontiguousarray(r))) for r in bad] == [np.inf] * 3        # a d that is not finite counts as +inf


def test_on_lo_and_hi_and_one_ulp_either_side(check):
    rng = np.random.default_rng(2)
    for mu, c2 in [(1.0, 0.25), (0.37, 0.0025), (9.5, 1e-4)] + [(float(m), float(c)) for m, c in zip(rng.uniform(1e-3, 50, 40), rng.uniform(1e-6, 1, 40))]:
        lo, hi = (float(v) for v in gr.bounds(mu, c2))
        assert check_weight(check, mu, c2, lo) == (1.0, 0)                                         # on lo: an inlier, not in the band
        assert check_weight(check, mu, c2, np.nextafter(lo, 0.0)) == (1.0, 0)
        w, band = check_weight(check, mu, c2, np.nextafter(lo, np.inf))
        assert band == 1 and 0.999999 < w <= 1.0
        assert check_weight(check, mu, c2, hi) == (0.0, 0)                                         # on hi: an outlier, not in the band
        assert check_weight(check, mu, c2, np.nextafter(hi, np.inf)) == (0.0, 0)
        w, band = check_weight(check, mu, c2, np.nextafter(hi, 0.0))
        assert band == 1 and 0.0 <= w < 1e-6
        assert check_weight(check, mu, c2, np.inf) == (0.0, 0)
        d = np.array([lo, hi, np.nextafter(lo, 0.0), np.nextafter(lo, np.inf), np.nextafter(hi, 0.0), np.nextafter(hi, np.inf), 0.5 * (lo + hi), np.inf])
        got = [check_weight(check, mu, c2, v) for v in d]
        w, band = gr.weights(gr.TLS, mu, c2, d)
        assert same_bits(np.array([g[0] for g in got]), w) and [g[1] for g in got] == [int(b) for b in band]
        _, wrong_band = gr.weights(gr.TLS, mu, c2, d, wrong="lo_strict")                           # `<` for `<=` at lo is refused
        assert [g[1] for g in got] != [int(b) for b in wrong_band]
        wg, _ = gr.weights(gr.GM, mu, c2, d)
        assert same_bits(np.array([gc.header_weight(check, gr.GM, mu, c2, v)[2] for v in d]), wg)


def check_weight(check, mu, c2, d):
    lo, hi, w, band = gc.header_weight(check, gr.TLS, mu, c2, d)
    assert (lo, hi) == tuple(float(v) for v in gr.bounds(mu, c2))
    return w, band


@pytest.mark.parametrize("dtype", DTYPES)
def test_twice_dmax_exactly_c2(check, dtype):
    a, thr = gc.half_c2_case()
    pairs = gc.flat_square(a, dtype)
    h = gc.header_fit(check, pairs, None, gr.TLS, thr, detail=True)
    assert same_bits(h["trace"][0, POSE], EYE) and (h["rounds"], h["status"], h["mu"]) == (0, gr.CONVERGED, 0.0)
    assert same_bits(h["weights"], np.ones(4, dtype)) and against_restatement(h, pairs, None, gr.TLS, thr, bound=False)
    below = float(np.nextafter(thr, 0.0))                       # c2 a step below 2 dmax: the rounds run
    assert below * below < 2.0 * (a * a)
    h = gc.header_fit(check, pairs, None, gr.TLS, below, detail=True)
    assert h["rounds"] >= 1 and h["mu"] > 0 and against_restatement(h, pairs, None, gr.TLS, below, bound=False)
    h = gc.header_fit(check, pairs, None, gr.GM, thr, detail=True)                                   # GM: mu = max(1, 1) = 1, one round
    assert (h["rounds"], h["status"], h["mu"]) == (1, gr.CONVERGED, 1.0) and against_restatement(h, pairs, None, gr.GM, thr, bound=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_round_that_trips_the_guard(check, dtype):
    rng = np.random.default_rng(5)
    pairs = rng.uniform(-1, 1, (6, 6)).astype(dtype)            # no motion fits these: TLS sheds pairs until fewer than three are left
    h = gc.header_fit(check, pairs, None, gr.TLS, 1e-3, detail=True)
    assert h["status"] == gr.GUARDED and 1 <= h["rounds"] < 128 and (h["weights"] > 0).sum() >= 3
    assert against_restatement(h, pairs, None, gr.TLS, 1e-3, bound=False)
    assert same_bits(h["w"][h["rounds"]].astype(dtype), h["weights"])                                # the weights of the last APPLIED round stand
    assert not against_restatement(h, pairs, None, gr.TLS, 1e-3, wrong="no_guard", bound=False)      # a missing guard is refused


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("loss", (gr.TLS, gr.GM))
def test_the_cap_and_the_mu_schedule(check, dtype, loss):
    rng = np.random.default_rng(6)
    pairs = gc.noisy_cloud(rng, 200, dtype)
    one = gc.header_fit(check, pairs, None, loss, 0.04, iterations=1, detail=True)
    assert (one["rounds"], one["status"]) == (1, gr.CAPPED) and against_restatement(one, pairs, None, loss, 0.04, iterations=1)
    full = gc.header_fit(check, pairs, None, loss, 0.04, detail=True)
    assert same_bits(full["trace"][:2], one["trace"][:2]) and full["rounds"] > 5 and full["status"] == gr.CONVERGED
    mus = full["trace"][1:full["rounds"] + 1, 0]
    if loss == gr.TLS:
        assert same_bits(mus[1:], mus[:-1] * 1.4)
        assert not against_restatement(full, pairs, None, loss, 0.04, wrong="mu_divided")            # mu divided where it is multiplied is refused
    else:
        assert mus[-1] == 1.0 and np.all(mus[:-1] > 1.0) and same_bits(mus[1:], np.maximum(1.0, mus[:-1] / 1.4))
    capped = gc.header_fit(check, pairs, None, loss, 0.04, iterations=full["rounds"])                # the last round meets its own rule AT the cap: status 0
    assert (capped["rounds"], capped["status"]) == (full["rounds"], gr.CONVERGED)
    for g in (1.05, 2.0, 16.0):
        h = gc.header_fit(check, pairs, None, loss, 0.04, growth=g, iterations=256, detail=True)
        assert against_restatement(h, pairs, None, loss, 0.04, growth=g, iterations=256)


@pytest.mark.parametrize("dtype", DTYPES)
def test_user_weights_that_make_a_row_not_live(check, dtype):
    rng = np.random.default_rng(7)
    x, y, idx = gc.rows_cloud(rng, 120, 30, dtype)
    n = x.shape[0]
    w = rng.uniform(0.5, 1.5, n).astype(dtype)
    off = rng.permutation(np.flatnonzero(rr.live_mask(x, y, idx)))[:9]
    w[off[:3]], w[off[3:6]], w[off[6:]] = 0.0, -1.0, np.nan
    assert not gr.live_mask(x, y, idx, w)[off].any() and gr.live_mask(x, y, idx, w).sum() == 120 - 9
    h = gc.header_call(check, x, y, idx, 0.04, weight=w)
    assert h["pairs"].shape[0] == 111 and np.all(h["weights"][off] == 0) and np.all(h["weights"][~gr.live_mask(x, y, idx, w)] == 0)
    dropped = idx.copy()
    dropped[off] = -1
    w1 = np.where(np.isfinite(w) & (w > 0), w, 1).astype(dtype)
    h2 = gc.header_call(check, x, y, dropped, 0.04, weight=w1)                                       # the same as dropping those rows
    assert same_bits(h["weights"], h2["weights"]) and same_bits(h["trace"], h2["trace"])
    h3 = gc.header_call(check, x, y, idx, 0.04, weight=w, x_rows=100)
    assert np.all(h3["weights"][100:] == 0) and h3["pairs"].shape[0] == gr.live_mask(x, y, idx, w, 100).sum()


def test_a_residual_that_is_not_finite(check):
    rng = np.random.default_rng(8)
    pairs = gc.noisy_cloud(rng, 60, np.float64, inlier_ratio=0.8)
    pairs[7, :3] = 1e200                                        # |C x|^2 overflows: d = +inf whatever the pose
    u = np.ones(60)
    u[7] = 1e-250                                               # ... and at this weight the pair does not disturb round 0
    for loss in (gr.TLS, gr.GM):
        h = gc.header_fit(check, pairs, u, loss, 0.04, detail=True)
        assert against_restatement(h, pairs, u, loss, 0.04, bound=False)
        assert h["rounds"] > 5 and h["status"] == gr.CONVERGED and np.isfinite(h["pose_last"]).all()
        assert np.all(h["d"][1:h["rounds"] + 1, 7] == np.inf) and h["weights"][7] == 0 and (h["weights"] > 0).sum() > 30
    # at weight 1 the pair owns round 0 and every residual overflows: dmax = 0
    h = gc.header_fit(check, pairs, None, gr.TLS, 0.04, detail=True)
    assert (h["rounds"], h["status"]) == (0, gr.CONVERGED) and against_restatement(h, pairs, None, gr.TLS, 0.04, bound=False)
    h = gc.header_fit(check, pairs, None, gr.GM, 0.04, detail=True)
    assert (h["rounds"], h["status"]) == (0, gr.GUARDED) and against_restatement(h, pairs, None, gr.GM, 0.04, bound=False)
    assert same_bits(h["weights"], np.ones(60))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", (0, 1, 2, 3))
def test_fewer_than_three_pairs(check, dtype, P):
    pairs = gc.noisy_cloud(np.random.default_rng(P), max(P, 1), dtype)[:P]
    for loss in (gr.TLS, gr.GM):
        h = gc.header_fit(check, pairs, None, loss, 0.04, detail=True)
        if P < 3:
            assert (h["rounds"], h["status"], h["mu"]) == (0, gr.TOO_FEW, 0.0) and np.all(h["weights"] == 0)
            assert same_bits(h["pose_last"], EYE.astype(dtype)) and not h["trace"].any()
        else:
            assert h["status"] != gr.TOO_FEW and against_restatement(h, pairs, None, loss, 0.04, bound=False)
        assert gr.gnc_ref(pairs, None, loss, 0.04)["status"] == (gr.TOO_FEW if P < 3 else h["status"])


# ------------------------------------------------------------------ recovery, on the g++ build
@pytest.mark.parametrize("case", gc.recovery_cases(), ids=lambda c: c[0] if isinstance(c, tuple) else None)
def test_recovery_on_the_host_build(check, case):
    name, a, thr, limit = case
    ls = gc.least_squares_error(a)
    assert ls > gc.LEAST_SQUARES_FLOOR                         # why a robust fit: least squares over every match is far off
    for loss in ("tls", "gm"):
        h = gc.header_call(check, a["x"], a["y"], a["idx"], thr, loss)
        err = rr.rotation_error(h["pose_last"][:9], a["C"])
        print("%s %s: rounds %d status %d, rotation error %.3g (limit %.3g), least squares %.3g" % (name, loss, h["rounds"], h["status"], err, limit, ls))
        assert err <= limit and h["status"] == gr.CONVERGED
        if loss == "tls" and name.startswith("compat"):
            assert np.array_equal(h["weights"] > 0, a["truth"]) and np.all(h["weights"][a["truth"]] == 1)     # exactly the true pairs, at weight 1


# ------------------------------------------------------------------ the Python front: ValueError before any device work
def _bad(*args, **kw):
    with pytest.raises(ValueError, match="gnc_correspondences"):
        gnc_correspondences(*args, **kw)


def test_argument_checks_of_the_python_function(check):
    x, y, idx = torch.zeros(5, 3), torch.zeros(7, 3), torch.zeros(5, dtype=torch.int64)
    for thr in (0, 0.0, -1.0, float("inf"), float("nan"), "0.1", None, True, torch.tensor(0.1), 1e-200, 1e200):
        _bad(x, y, idx, thr)
    for loss in ("huber", "TLS", 0, None, True, b"tls"):
        _bad(x, y, idx, 0.1, loss=loss)
    for g in (1, 1.0, 0.5, -2.0, 16.5, float("inf"), float("nan"), "1.4", None, True):
        _bad(x, y, idx, 0.1, growth=g)
    for it in (0, -1, 257, 10.0, True, None, "8"):
        _bad(x, y, idx, 0.1, iterations=it)
    for r in (1, 0, None, "yes"):
        _bad(x, y, idx, 0.1, return_info=r)
    # the forms and checks of align_correspondences
    _bad(x, y, idx.float(), 0.1)
    _bad(x, y, idx[:4], 0.1)
    _bad(x, y, idx + 7, 0.1)
    _bad(x, y, idx, 0.1, weight=torch.ones(5, dtype=torch.float64))
    _bad(x, y, idx, 0.1, weight=torch.ones(4))
    _bad(x[:, :2], y, idx, 0.1)
    _bad([x], [y], idx, 0.1)
    _bad(x, y, idx, 0.1, x_rows=torch.tensor([3]))
    _bad(x[None], y[None], idx[None], 0.1, x_rows=torch.tensor([6]))
    _bad(x.half(), y.half(), idx, 0.1)
    # the header's own check agrees with the Python one
    for args, bad in (((0, 0.1, 1.4, 128), 0), ((1, 0.1, 16.0, 256), 0), ((2, 0.1, 1.4, 8), 1), ((0, 0.0, 1.4, 8), 1), ((0, 1e-200, 1.4, 8), 1),
                      ((0, 1e200, 1.4, 8), 1), ((0, float("nan"), 1.4, 8), 1), ((0, 0.1, 1.0, 8), 1), ((0, 0.1, 16.5, 8), 1),
                      ((0, 0.1, float("nan"), 8), 1), ((0, 0.1, 1.4, 0), 1), ((0, 0.1, 1.4, 257), 1)):
        assert check.gc_bad_arguments(*args) == bad, args
