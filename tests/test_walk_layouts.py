"""The window model of tests/walk_layouts.py against the kernels' sources, and the layouts against the conditions that make them tests of the
out-of-window paths (no GPU: the model and a float64 neighbour search on the host)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import walk_layouts as wl  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dicp_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constant(text, struct, ctype, block):
    m = re.search(r"template <> struct %s<%s>\s*\{ static constexpr int v = ([A-Z0-9+* ]+); \};" % (struct, ctype), text)
    assert m, "%s<%s> not found" % (struct, ctype)
    value = 0                                               # a sum of products of integers and BLOCK
    for term in m.group(1).split("+"):
        prod = 1
        for f in term.split("*"):
            prod *= block if f.strip() == "BLOCK" else int(f)
        value += prod
    return value


def test_window_constants_match_the_sources():
    common, knn, nrm = _text("dicp_common.h"), _text("knn_points.hip"), _text("normals.hip")
    m = re.search(r"constexpr int BLOCK = (\d+);", common)
    assert m and int(m.group(1)) == wl.BLOCK
    for ctype, dt in (("float", np.float32), ("double", np.float64)):
        H, W = wl.HALO[np.dtype(dt)], wl.win_rows(dt)
        assert _constant(knn, "WinHalo", ctype, wl.BLOCK) == H
        assert _constant(knn, "WinRows", ctype, wl.BLOCK) == W
        assert _constant(knn, "BwdRows", ctype, wl.BLOCK) == W
        assert _constant(nrm, "WalkHalo", ctype, wl.BLOCK) == H
        assert _constant(nrm, "BwdHalo", ctype, wl.BLOCK) == H
    assert (wl.win_rows(np.float32), wl.win_rows(np.float64)) == (2304, 1280)
    # the window expressions the model repeats, as the kernels state them
    for line in ("wlo = max(span[0] - H, 0);", "whi = min(min(span[1] + H, mb), wlo + W);",
                 "const int wlo = span[1] >= 0 ? span[0] : 0, whi = span[1] >= 0 ? min(span[1] + 1, wlo + W) : 0, wn = (whi - wlo) * 3;",
                 "constexpr int H = WinHalo<T>::v, W = WinRows<T>::v;", "constexpr int W = BwdRows<T>::v;",
                 "if (p.x == p.x) { atomicMin(&span[0], pos); atomicMax(&span[1], pos); }"):
        assert line in knn, line
    for line in ("const int wlo = max(s0 - H, 0), whi = min(s0 + BLOCK + H, mb);", "__shared__ T4 win[BLOCK + 2 * H];",
                 "const int wlo = max(s0 - H, 0), whi = min(s0 + BLOCK + H, mb), wn = (whi - wlo) * 3;", "__shared__ T acc[(BLOCK + 2 * H) * 3];",
                 "constexpr int H = WalkHalo<T>::v;", "constexpr int H = BwdHalo<T>::v;"):
        assert line in nrm, line


def test_model_neighbours_against_the_brute_force():
    x, y = wl.cube(700, 3), wl.cube(900, 4)
    for X, Y, k in ((x, y, 8), (wl.wall(500, 1), wl.wall(600, 2), 16), (x, y[:5], 8), (x[:3], y, 1)):
        got = wl.model_neighbours(X, Y, k)
        _, ref = wl.knn_oracle(X, Y, k)
        assert np.array_equal(np.sort(got, 1), np.sort(ref, 1))


def test_model_on_a_hand_made_case():
    # float64: H = 512, W = 1280.  3000 targets at x = 0, 1, 2, ...; one block of two queries at x = 100.5 and x = 2500.5, k = 2
    y = np.stack([np.arange(3000.0), np.zeros(3000), np.zeros(3000)], 1)
    x = np.array([[100.5, 0, 0], [2500.5, 0, 0]])
    idx = np.array([[100, 101], [2500, 2501]])
    w = wl.knn_windows(x, y, 2, np.float64, idx)
    # forward: span [101, 2501] -> wlo 0, whi min(3013, 3000, 1280): the second query's rows are outside, the window is capped
    assert w.fwd_outside.tolist() == [[False, False], [True, True]] and w.capped_fwd == 1
    # backward: used slots 100 .. 2501 -> [100, 1380), capped
    assert w.bwd_outside.tolist() == [[False, False], [True, True]] and w.capped_bwd == 1
    assert w.indegree[100] == 1 and w.indegree.sum() == 4
    # the same in the original query order reversed
    w = wl.knn_windows(x[::-1], y, 2, np.float64, idx[::-1])
    assert w.bwd_outside.tolist() == [[True, True], [False, False]]
    # normals: 3000 rows on a line, the last neighbour of row 0 set to row 767 / 768: the window of block 0 is [0, 256 + 512)
    nbr = np.tile(np.arange(3000)[:, None], (1, 3))
    nbr[0, 2], nbr[1, 2] = 767, 768
    wn = wl.normals_windows(y, 3, np.float64, nbr)
    assert not wn.bwd_outside[0].any() and wn.bwd_outside[1].tolist() == [False, False, True] and wn.bwd_outside.sum() == 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", wl.KNN_LAYOUTS)
def test_knn_layouts_meet_their_conditions(name, dtype):
    x, y, k = wl.knn_layout(name, dtype)
    w = wl.knn_windows(x, y, k, dtype)
    print("%s %s: fwd outside %.3f, bwd outside %.3f, capped fwd %d bwd %d of %d blocks, max in-degree %d"
          % (name, np.dtype(dtype).name, w.share("fwd"), w.share("bwd"), w.capped_fwd, w.capped_bwd, w.blocks, w.indegree.max()))
    wl.check_knn_conditions(name, dtype, w)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", wl.NORMALS_LAYOUTS)
def test_normals_layouts_meet_their_conditions(name, dtype):
    P, k = wl.normals_layout(name)
    w = wl.normals_windows(P, k, dtype)
    print("normals %s %s: bwd outside %.3f, max in-degree %d" % (name, np.dtype(dtype).name, w.share(), w.indegree.max()))
    wl.check_normals_conditions(name, dtype, w)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_gradient_bounds_bite(dtype):
    """knn_grad_check on gradients formed on the host the way the kernel forms them (terms in double; x summed in double and rounded once, y
    rounded per term and summed in the dtype): they pass, and a NaN, a halved term or a dropped term in either gradient does not."""
    dt = np.dtype(dtype)
    x, y, k = wl.knn_layout("edge_m+257", dtype)
    X, Y = x.astype(dt), y.astype(dt)
    _, idx = wl.knn_oracle(X, Y, k)
    g = np.random.default_rng(7).standard_normal(idx.shape).astype(dt)
    t = 2 * g.astype(np.float64)[:, :, None] * (X.astype(np.float64)[:, None, :] - Y[idx].astype(np.float64))
    gx = t.sum(1).astype(dt)
    gy = np.zeros_like(Y)
    np.add.at(gy, idx.reshape(-1), (-t).astype(dt).reshape(-1, 3))
    wl.knn_grad_check(X, Y, idx, g, gx, gy, dtype)
    i, j = 5, 2
    l = idx[i, j]
    for what, dx, dy in (("halved", -0.5 * t[i, j], 0.5 * t[i, j]), ("dropped", -t[i, j], t[i, j]), ("NaN", np.nan, np.nan)):
        bx, by = gx.copy(), gy.copy()
        bx[i] = (bx[i].astype(np.float64) + dx).astype(dt)
        by[l] = (by[l].astype(np.float64) + dy).astype(dt)
        with pytest.raises(AssertionError, match="x-gradient"):
            wl.knn_grad_check(X, Y, idx, g, bx, gy, dtype, what)
        with pytest.raises(AssertionError, match="y-gradient"):
            wl.knn_grad_check(X, Y, idx, g, gx, by, dtype, what)
    by = gy.copy()
    by[np.flatnonzero(np.bincount(idx.reshape(-1), minlength=Y.shape[0]) == 0)[0], 1] = np.nan       # a row no list holds
    with pytest.raises(AssertionError, match="y-gradient"):
        wl.knn_grad_check(X, Y, idx, g, gx, by, dtype)
    with pytest.raises(AssertionError):
        wl.assert_within(np.array([np.nan]), np.array([0.0]), np.array([1.0]), "nan")
