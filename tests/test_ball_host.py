"""CPU checks of ball_query (dicp_amd/ball.py) that need no GPU.

``dicp_amd/csrc/dicp_ball.h`` -- the search half-width R, the plan of a grid (origin, cell edges, key widths), the cell keys, the range
enumeration and the per-query scan of the HIP kernels -- is compiled with g++ through tests/hostcheck/ball_check.cpp, run serially on a
grid built on the host and held to the numpy brute force tests/ball_ref.py: index for index, d2 bit for bit, counts exactly, on the clouds
of the GPU tests.  The inputs are shown to do their job (a span of 4 cells, the enlarged edge, candidates outside the query's cell), the
comparison is shown to refuse a reference that is wrong by one neighbour or by `<` for `<=`, and the argument checks of ``ball_query``
run before any device work.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.ball import ball_query

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ball_clouds as bc  # noqa: E402
from ball_ref import ball_ref, same  # noqa: E402
import hostbuild  # noqa: E402

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def check():
    lib = hostbuild.build("ball_check.cpp", "ball_check", ("-Wall",))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.bc_run_f32.argtypes = [vp, i32, i32, i32, vp, i32, i32, i32, ctypes.c_float, i32, vp, vp, vp, vp]
    lib.bc_run_f64.argtypes = [vp, i32, i32, i32, vp, i32, i32, i32, ctypes.c_double, i32, vp, vp, vp, vp]
    lib.bc_run_f32.restype = lib.bc_run_f64.restype = None
    lib.bc_R_f32.argtypes, lib.bc_R_f32.restype = [ctypes.c_float], ctypes.c_float
    lib.bc_R_f64.argtypes, lib.bc_R_f64.restype = [ctypes.c_double], ctypes.c_double
    return lib


STATS = ("span_x", "span_y", "span_z", "enlarged", "flat", "other_cell", "visited", "live")


def _header(lib, x, y, radius, k, x_rows=None, y_rows=None):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    n, m = x.shape[0], y.shape[0]
    d2 = np.zeros((n, k), dtype=x.dtype)
    idx = np.zeros((n, k), dtype=np.int64)
    counts = np.zeros(n, dtype=np.int32)
    stats = np.zeros(8, dtype=np.int64)
    fn = lib.bc_run_f32 if x.dtype == np.float32 else lib.bc_run_f64
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fn(p(x), n, x.shape[1], n if x_rows is None else x_rows, p(y), m, y.shape[1], m if y_rows is None else y_rows,
       float(x.dtype.type(radius)), k, p(d2), p(idx), p(counts), p(stats))
    return (d2, idx, counts), dict(zip(STATS, stats.tolist()))


def _hold(lib, x, y, radius, ks=bc.KS, **rows):
    ref = ball_ref(x, y, radius, max(ks), **rows)
    stats = None
    for k in ks:
        got, stats = _header(lib, x, y, radius, k, **rows)
        bad = same(got, (ref[0][:, :k], ref[1][:, :k], ref[2]))
        assert bad is None, "k=%d: %s" % (k, bad)
    return ref, stats


@pytest.mark.parametrize("dtype", DTYPES)
def test_header_matches_reference_on_random_cubes(check, dtype):
    """fails without dicp_ball.h"""
    seen = set()
    for n, m in bc.RANDOM_SHAPES:
        x, y = bc.random_pair(n, m, dtype)
        for r in bc.RANDOM_RADII:
            ref, _ = _hold(check, x, y, r)
            c = ref[2]
            seen |= {"zero"} if (c == 0).any() else set()
            seen |= {"some"} if ((c > 0) & (c <= 8)).any() else set()
            seen |= {"over"} if (c > 32).any() else set()
            if r == 2.0:
                assert (c == m).all()
    assert seen == {"zero", "some", "over"}


@pytest.mark.parametrize("dtype", DTYPES)
def test_header_matches_reference_on_the_lattice(check, dtype):
    centre = 171
    want = {1.0: 7, 1.5: 19, 2.0: 33}
    for name, x, y, r in bc.lattice_cases(dtype):
        ref, stats = _hold(check, x, y, r)
        if name.startswith("lattice r=") and r in want:
            assert ref[2][centre] == want[r], name
        assert stats["other_cell"] > 0, name
    s2 = float(np.sqrt(dtype(2)))
    assert ball_ref(bc.lattice(dtype), bc.lattice(dtype), s2, 32)[2][centre] == (7 if dtype == np.float32 else 19)    # the dtype's own rounding of r2 decides
    L = bc.lattice(dtype)
    D = (L[:, None, :] - L[None, :, :]).astype(np.float64)
    D = (D * D).sum(-1)
    assert (D == 1.0).sum() == 1764 and (D == 4.0).sum() == 1470          # pairs that sit on the bound exactly


@pytest.mark.parametrize("dtype", DTYPES)
def test_header_matches_reference_on_degenerate_layouts(check, dtype):
    for name, x, y, r in bc.degenerate_cases(dtype):
        ref, stats = _hold(check, x, y, r)
        if name == "300 copies":
            assert ref[2].tolist() == [300, 300, 0]
        if name == "two clusters":
            assert stats["enlarged"] == 1 and stats["flat"] == 0 and (ref[2] > 1).any() and stats["visited"] < x.shape[0] * y.shape[0] // 2
        if name == "underflow":
            assert ref[2].tolist() == [2]
        if name == "far queries":
            assert ref[2][:4].tolist() == [0, 0, 0, 0] and ref[2][5] > 0
        if name == "wall":
            assert stats["enlarged"] == 0 and stats["visited"] < x.shape[0] * y.shape[0] // 10


@pytest.mark.parametrize("dtype", DTYPES)
def test_header_on_non_finite_and_ragged_rows(check, dtype):
    x, y = bc.nonfinite_pair(dtype)
    ref, stats = _hold(check, x, y, 0.15)
    assert stats["live"] == 900 - 4
    assert ref[2][[0, 7, 150]].tolist() == [0, 0, 0] and not np.isin(ref[1], [5, 17, 400, 899]).any()
    _hold(check, x, y, 0.15, x_rows=200, y_rows=650)
    _hold(check, x, y, 0.15, x_rows=0, y_rows=650)
    _hold(check, x, y, 0.15, x_rows=200, y_rows=0)
    _hold(check, np.concatenate([x, x], 1), np.concatenate([y, y + 1], 1), 0.15, ks=(8,))          # 6 columns: 0:3 are used
    big = np.array([[3.0e38, 0, 0], [-3.0e38, 0, 0], [0, 0, 0], [0, 1, 0]], dtype=dtype)           # float32: the extent overflows -> one cell
    ref, stats = _hold(check, big[2:], big, 1.5, ks=(8,))
    assert ref[2].tolist() == [2, 2] and stats["flat"] == (1 if dtype == np.float32 else 0)
    big = np.array([[1.0e19, 0, 0], [-1.0e19, 0, 0], [0, 0, 0], [0, 1, 0]], dtype=dtype)
    ref, _ = _hold(check, big, big, 1.0e30, ks=(8,))                                               # float32: r2 = +inf, only finite d2 count
    assert ref[2].tolist() == ([3, 3, 4, 4] if dtype == np.float32 else [4, 4, 4, 4])


def test_inputs_reach_a_span_of_four_cells(check):
    spans = 0
    for name, x, y, r in bc.lattice_cases(np.float32) + bc.degenerate_cases(np.float32):
        _, stats = _header(check, x, y, r, 8)
        if not stats["enlarged"]:
            spans = max(spans, stats["span_x"], stats["span_y"], stats["span_z"])
    assert spans >= 4


@pytest.mark.parametrize("dtype", DTYPES)
def test_search_half_width(check, dtype):
    """R is at least radius (1 + 6u) and at least the underflow floor, and adversarial pairs at |dx| = r (1 +- few ulp) stay inside it"""
    fn = check.bc_R_f32 if dtype == np.float32 else check.bc_R_f64
    u = np.finfo(dtype).eps / 2
    rng = np.random.default_rng(9)
    for r in [1e-25, 1e-3, 0.02, 1.0, 2.5e3] + (10.0 ** rng.uniform(-6, 6, 50)).tolist():
        r = dtype(r)
        R = dtype(fn(float(r)))
        assert float(R) >= float(r) * (1 + 6 * u) and float(R) >= (2.0 ** -49 if dtype == np.float32 else 2.0 ** -483)
        p = (rng.uniform(-1, 1, 2000) * 10.0 ** rng.integers(0, 7, 2000)).astype(dtype)
        ulps = rng.integers(-4, 5, 2000)
        yv = p + r
        for _ in range(4):
            yv = np.where(ulps > 0, np.nextafter(yv, dtype(np.inf)), np.where(ulps < 0, np.nextafter(yv, dtype(-np.inf)), yv))
            ulps = ulps - np.sign(ulps)
        e = yv - p
        cand = (e * e) <= r * r
        assert cand.any()
        assert (np.abs(yv[cand].astype(np.longdouble) - p[cand].astype(np.longdouble)) <= np.longdouble(R)).all()
        assert ((p[cand] - R) <= yv[cand]).all() and (yv[cand] <= (p[cand] + R)).all()


def test_comparison_refuses_a_wrong_reference():
    L = bc.lattice(np.float32)
    true = ball_ref(L, L, 1.0, 8)
    assert same(true, true) is None
    assert same(true, ball_ref(L, L, 1.0, 8, strict=True)) is not None            # `<` in place of `<=`: the lattice sits on the bound
    assert same(true, ball_ref(L, L, 1.0, 8, drop=(171, 3))) is not None          # one neighbour removed
    x, y = bc.random_pair(700, 5000, np.float32)
    true = ball_ref(x, y, 0.1, 8)
    i = int(np.flatnonzero(true[2] > 8)[0])
    assert same(true, ball_ref(x, y, 0.1, 8, drop=(i, 8))) is not None           # a neighbour beyond the list: only counts shows it
    assert same(true, ball_ref(x, y, 0.1, 8, strict=True)) is None                # (no pair of a random cloud sits on the bound)


def test_entry_points_reject_bad_arguments():
    """null pointers, a bad dtype, bad shapes, misaligned buffers: refused before any launch (no GPU touched)"""
    from dicp_amd import _lib
    _lib.build()
    lib = _lib.load()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)
    assert lib.dicp_ball_grid_slots(1) == 2 and lib.dicp_ball_grid_slots(5000) == 8192 and lib.dicp_ball_grid_slots(16384) == 16384
    assert lib.dicp_ball_grid_slots(0) == 0 and lib.dicp_ball_grid_slots(2 ** 30 + 1) == 0 and lib.dicp_ball_plan_bytes() % 8 == 0

    def call(fn, good, **kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return fn(*a)
    # dicp_ball_grid_build(dtype, pts, c, rows, N, m, radius, order_by, plans, keys, perm, rows4, stream)
    good = [0, one, 3, None, 1, 10, one, None, one, one, one, one, None]
    build = lambda **kw: call(lib.dicp_ball_grid_build, good, **kw)  # noqa: E731
    assert [build(**{"a%d" % i: None}) for i in (1, 6, 8, 9, 10, 11)] == [1] * 6
    assert build(a7=one) == 1 and build(a7=one, a6=None, a8=None) == 1                      # ordering by another grid takes no plans / rows4
    assert build(a0=7) == 3 and build(a4=0) == 2 and build(a5=0) == 2 and build(a2=2) == 2 and build(a5=2 ** 30 + 1) == 2
    assert build(a1=odd) == 5 and build(a9=odd) == 5 and build(a11=ctypes.c_void_p(264)) == 5
    # dicp_ball_query(dtype, x, cx, n, x_keys, x_perm, y_plans, y_keys, y_perm, y_rows4, m, N, k, d2, idx, counts, workspace, bytes, visited, stream)
    good = [0, one, 3, 10, one, one, one, one, one, one, 20, 1, 8, one, one, one, one, 1 << 20, None, None]
    query = lambda **kw: call(lib.dicp_ball_query, good, **kw)  # noqa: E731
    assert [query(**{"a%d" % i: None}) for i in (1, 4, 5, 6, 7, 8, 9, 13, 14, 15, 16)] == [1] * 11
    assert query(a0=2) == 3 and query(a3=0) == 2 and query(a10=0) == 2 and query(a11=0) == 2 and query(a2=2) == 2
    assert query(a12=0) == 2 and query(a12=33) == 2 and query(a17=16) == 2                  # k outside [1, 32]; a workspace too small
    assert query(a13=odd) == 5 and query(a14=ctypes.c_void_p(260)) == 5
    assert lib.dicp_ball_query_workspace_bytes(0, 1, 10, 8) >= 320 and lib.dicp_ball_query_workspace_bytes(0, 1, 10, 33) == 0
    assert lib.dicp_ball_query_workspace_bytes(5, 1, 10, 8) == 0 and lib.dicp_ball_query_workspace_bytes(0, 1, 0, 8) == 0
    # dicp_ball_query_backward(dtype, g_d2, x, cx, n, y_rows4, y_perm, m, cy, N, k, fwd_workspace, grad_x, grad_y, stream)
    good = [0, one, one, 3, 10, one, one, 20, 3, 1, 8, one, one, one, None]
    bwd = lambda **kw: call(lib.dicp_ball_query_backward, good, **kw)  # noqa: E731
    assert [bwd(**{"a%d" % i: None}) for i in (1, 2, 5, 6, 11)] == [1] * 5
    assert bwd(a0=-1) == 3 and bwd(a3=2) == 2 and bwd(a8=2) == 2 and bwd(a4=0) == 2 and bwd(a7=0) == 2 and bwd(a9=0) == 2 and bwd(a10=40) == 2
    assert bwd(a12=odd) == 5 and bwd(a12=None, a13=None) == 0                               # nothing asked for: nothing launched


# ---------------------------------------------------------------- argument checks (before any device work)

def _raises(*a, **kw):
    with pytest.raises(ValueError):
        ball_query(*a, **kw)


def test_ball_query_rejects_bad_arguments():
    x, y = torch.rand(5, 3), torch.rand(4, 3)
    for r in (0, 0.0, -1.0, float("inf"), float("nan"), [0.1], (0.1,), "0.1", None, True, torch.tensor([0.1]), torch.tensor(0.0),
              torch.tensor(float("nan")), torch.tensor(1), 1e-60, 1e39, 10 ** 400):
        _raises(x, y, r)
    for k in (0, 33, -1, 1.0, True, "8", None):
        _raises(x, y, 0.1, k=k)
    _raises(x, y.unsqueeze(0), 0.1)                         # mismatched forms
    _raises([x], y, 0.1)
    _raises(x.unsqueeze(0), [y], 0.1)
    _raises(x, y.double(), 0.1)
    _raises(x[:, :2], y, 0.1)
    _raises(x.half(), y.half(), 0.1)
    _raises(x, y, 0.1, x_rows=torch.tensor([3]))            # row counts need a padded batch
    _raises(x.unsqueeze(0), y.unsqueeze(0), 0.1, y_rows=torch.tensor([5]))
    _raises(x.unsqueeze(0), y.unsqueeze(0), 0.1, x_rows=torch.tensor([1.0]))
    _raises(torch.rand(2, 5, 3), torch.rand(3, 4, 3), 0.1)
    _raises([], [], 0.1)
    _raises("x", y, 0.1)
