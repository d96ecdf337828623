"""CPU checks of the cell-grid k-NN search (knn_points / chamfer_distance with method="grid") that need no GPU.

``dicp_amd/csrc/dicp_gridknn.h`` -- the density plan, the cell keys and the per-query scan of the HIP kernels -- is compiled with g++ through
tests/hostcheck/gridknn_check.cpp, run serially on a grid built on the host and held to the numpy brute force walk_layouts.knn_oracle:
idx index for index, d2 bit for bit, on the clouds of the GPU tests.  The inputs are shown to do their job from the scan's own statistics
(growth passes, closing passes that reach new cells, enlarged and flat plans, whole-grid exhaustion), the comparison is shown to refuse a
reference with one neighbour swapped, the scan is shown to be local, and the argument checks of ``method=`` run before any device work.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.knn import chamfer_distance, knn_points

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ball_clouds as bc  # noqa: E402
import gridknn_host as gh  # noqa: E402

DTYPES = [np.float32, np.float64]


def _hold(x, y, ks=gh.KS, edge=0.0, **rows):
    """the header at every k against the brute force at the largest (its leading columns are the smaller k's) -> stats by k"""
    ref = gh.reference(x, y, max(ks), **rows)
    stats = {}
    for k in ks:
        got, stats[k] = gh.header(x, y, k, edge=edge, **rows)
        bad = gh.same(got, (ref[0][:, :k], ref[1][:, :k]))
        assert bad is None, "k=%d: %s" % (k, bad)
        assert stats[k]["max_passes"] <= stats[k]["bound"]
    return ref, stats


@pytest.mark.parametrize("dtype", DTYPES)
def test_header_matches_brute_force_on_random_cubes(dtype):
    """fails without dicp_gridknn.h"""
    for n, m in bc.RANDOM_SHAPES:
        x, y = bc.random_pair(n, m, dtype)
        _, stats = _hold(x, y)
        if (n, m) == (700, 5000):
            # locality: about two rows per cell and a few dozen cells, not a brute force in disguise
            assert stats[8]["visited"] / n < m / 4 and stats[8]["visited"] / n < 500
            assert stats[1]["visited"] / n < 100 and stats[32]["visited"] / n < 500
            assert stats[8]["enlarged"] == 0 and stats[8]["flat"] == 0 and stats[8]["live"] == m


@pytest.mark.parametrize("dtype", DTYPES)
def test_header_on_the_lattice_and_the_degenerate_layouts(dtype):
    """ties at equal d2 across cells (the lattice), one cell, lines, a wall, clusters, far queries, k above the row count, the flat plan"""
    seen = {}
    for name, x, y in gh.all_cases(dtype):
        ref, stats = _hold(x, y)
        seen[name] = (ref, stats)
    L = seen["lattice r=1.0"][0]
    assert (L[0][171, :7] == [0, 1, 1, 1, 1, 1, 1]).all() and L[1][171, :7].tolist() == [171, 122, 164, 170, 172, 178, 220]   # six ties, by index
    assert seen["300 copies"][0][1][0, :8].tolist() == list(range(8)) and seen["300 copies"][1][8]["whole"] == 3
    for name in ("line along z", "line along x", "wall"):                     # the rule sees the degenerate axes: still a few rows per cell
        st = seen[name][1][8]
        assert st["visited"] / seen[name][0][0].shape[0] < 100 and st["flat"] == 0, name
    ref, stats = seen["k above the live rows"]
    assert (ref[1][:, 4:] == -1).all() and (ref[1][:, :4] >= 0).all() and stats[8]["whole"] == 50 and stats[8]["live"] == 4
    ref, stats = seen["small cluster facing a far one"]
    assert (ref[1][:40, :5] < 5).all() and (ref[1][:40, 5:8] >= 5).all()      # 5 near rows, then rows of the far cluster
    assert stats[8]["grew"] >= 40
    ref, stats = seen["queries 1e6 extents away"]
    assert (ref[1][:, 0] >= 0).all() and stats[8]["max_passes"] <= 4          # the gap jump: not 20 doublings
    if dtype == np.float32:
        ref, stats = seen["queries at 1e30"]
        assert (ref[1][:4] == -1).all() and (ref[1][4] >= 0).all() and stats[8]["whole"] >= 4        # d2 overflows: no candidate, bounded passes
        assert stats[8]["max_passes"] <= 4
    assert seen["extent 3e38"][1][8]["flat"] == (1 if dtype == np.float32 else 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_header_on_non_finite_empty_and_ragged_rows(dtype):
    x, y = bc.nonfinite_pair(dtype)
    ref, stats = _hold(x, y)
    assert stats[8]["live"] == 900 - 4
    assert (ref[1][[0, 7, 150]] == -1).all() and not np.isin(ref[1], [5, 17, 400, 899]).any()
    _hold(x, y, x_rows=200, y_rows=650)
    _hold(x, y, x_rows=0, y_rows=650)
    ref, _ = _hold(x, y, x_rows=200, y_rows=0)                                # an empty cloud
    assert (ref[1] == -1).all() and np.isinf(ref[0]).all()
    _hold(np.concatenate([x, x], 1), np.concatenate([y, y + 1], 1), ks=(8,))  # 6 columns: 0:3 are used


@pytest.mark.parametrize("dtype", DTYPES)
def test_any_edge_is_exact_and_the_fit_loop_enlarges(dtype):
    """The scan is exact at every starting edge, not only the rule's: far too small (many growth passes; on the two clusters 2e6 apart
    extent / edge needs more than 63 key bits, so the fit loop enlarges the edge), far too large (one cell) and the rule's own"""
    x, y = bc.random_pair(300, 2000, dtype, seed=2)
    _, tiny = _hold(x, y, edge=1e-4)
    assert tiny[8]["grew"] == 300 and tiny[8]["max_passes"] >= 8 and tiny[8]["enlarged"] == 0
    _, huge = _hold(x, y, edge=50.0)
    assert huge[8]["whole"] == 300 and huge[8]["visited"] == 300 * 2000
    cx, cy, _ = bc.cluster_pair(dtype)
    _, st = _hold(cx, cy, edge=1e-9 if dtype == np.float64 else 1e-3)
    assert st[8]["enlarged"] == 1 and st[8]["flat"] == 0
    _, st = _hold(cx, cy)                                                     # the rule's edge on the same cloud: two cells, nothing to enlarge
    assert st[8]["enlarged"] == 0 and st[8]["flat"] == 0


def test_inputs_reach_every_end_of_the_scan():
    """some query needs more than one growth pass, some closing pass feeds rows of cells outside the growth's box, some plan is enlarged,
    some is flat, some query ends on the whole grid -- and most end before it"""
    grew = closed = whole = early = flat = enlarged = 0
    for dtype in DTYPES:
        cases = [(x, y) for _, x, y in gh.all_cases(dtype)] + [bc.random_pair(n, m, dtype) for n, m in bc.RANDOM_SHAPES]
        for x, y in cases:
            _, st = gh.header(x, y, 8)
            grew += st["grew"]
            closed += st["closed"]
            whole += st["whole"]
            early += x.shape[0] - st["whole"]
            flat += st["flat"]
            enlarged += st["enlarged"]
    assert grew > 100 and closed > 100 and whole > 50 and early > 1000 and flat == 1 and enlarged >= 1


def test_comparison_refuses_a_wrong_reference():
    x, y = bc.random_pair(700, 5000, np.float32)
    true = gh.reference(x, y, 8)
    got, _ = gh.header(x, y, 8)
    assert gh.same(got, true) is None
    d2, idx = true[0].copy(), true[1].copy()
    idx[123, [2, 3]] = idx[123, [3, 2]]                                       # one pair of neighbours swapped
    assert gh.same(got, (true[0], idx)) is not None
    d2[123, 2] = np.nextafter(d2[123, 2], np.float32(np.inf))                 # one bit of one distance
    assert gh.same(got, (d2, true[1])) is not None
    L = bc.lattice(np.float32)
    true = gh.reference(L, L, 8)
    idx = true[1].copy()
    idx[171, [1, 2]] = idx[171, [2, 1]]                                       # two rows at the same d2 in the wrong order
    assert gh.same(gh.header(L, L, 8)[0], (true[0], idx)) is not None


def test_entry_points_reject_bad_arguments():
    """null pointers, a bad dtype, bad shapes, misaligned buffers: refused before any launch (no GPU touched)"""
    from dicp_amd import _lib
    _lib.build()
    lib = _lib.load()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)

    def call(fn, good, **kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return fn(*a)
    # dicp_knn_grid_build(dtype, pts, c, rows, N, m, plans, keys, perm, rows4, stream)
    good = [0, one, 3, None, 1, 10, one, one, one, one, None]
    build = lambda **kw: call(lib.dicp_knn_grid_build, good, **kw)  # noqa: E731
    assert [build(**{"a%d" % i: None}) for i in (1, 6, 7, 8, 9)] == [1] * 5
    assert build(a0=7) == 3 and build(a4=0) == 2 and build(a5=0) == 2 and build(a2=2) == 2 and build(a5=2 ** 30 + 1) == 2
    assert build(a1=odd) == 5 and build(a3=odd) == 5 and build(a7=odd) == 5 and build(a9=ctypes.c_void_p(264)) == 5
    # dicp_knn_grid_query(dtype, x, cx, n, x_keys, x_perm, y_plans, y_keys, y_perm, y_rows4, m, N, k, d2, idx, workspace, bytes, visited, passes, stream)
    good = [0, one, 3, 10, one, one, one, one, one, one, 20, 1, 8, one, one, one, 1 << 20, None, None, None]
    query = lambda **kw: call(lib.dicp_knn_grid_query, good, **kw)  # noqa: E731
    assert [query(**{"a%d" % i: None}) for i in (1, 4, 5, 6, 7, 8, 9, 13, 14, 15)] == [1] * 10
    assert query(a0=2) == 3 and query(a3=0) == 2 and query(a10=0) == 2 and query(a11=0) == 2 and query(a2=2) == 2
    assert query(a12=0) == 2 and query(a12=33) == 2 and query(a16=16) == 2                  # k outside [1, 32]; a workspace too small
    assert query(a13=odd) == 5 and query(a14=ctypes.c_void_p(260)) == 5 and query(a17=ctypes.c_void_p(260)) == 5 and query(a18=ctypes.c_void_p(260)) == 5
    assert lib.dicp_abi_version() == 11


def test_method_is_checked_before_any_device_work():
    x, y = torch.rand(5, 3), torch.rand(4, 3)
    for method in ("Grid", "cells", "", None, 1, True, b"grid"):
        with pytest.raises(ValueError, match='"walk" or "grid"'):
            knn_points(x, y, k=2, method=method)
        with pytest.raises(ValueError, match='"walk" or "grid"'):
            chamfer_distance(x, y, method=method)
    for method in ("walk", "grid"):                                            # the other checks come first, whatever the method
        for bad in (dict(k=0), dict(k=33), dict(k=1.0)):
            with pytest.raises(ValueError):
                knn_points(x, y, method=method, **bad)
        with pytest.raises(ValueError):
            knn_points(x, y.double(), method=method)
        with pytest.raises(ValueError):
            knn_points(x, y.unsqueeze(0), method=method)
        with pytest.raises(ValueError):
            knn_points(x[:, :2], y, method=method)
        with pytest.raises(ValueError):
            chamfer_distance(x, y, reduction="median", method=method)
        with pytest.raises(ValueError):
            chamfer_distance([x], y, method=method)
