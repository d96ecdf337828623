"""CPU checks of the neighbourhood feature operators (dicp_amd/group.py) that need no GPU.

``dicp_amd/csrc/dicp_group.h`` -- the per-slot rules of the HIP kernels -- is compiled with g++ through tests/hostcheck/group_check.cpp,
run in a serial loop and held to the numpy restatement tests/group_ref.py: liveness, the gather and the centre subtraction bit for
bit, the interpolation and its d2 gradient within their derived bounds against float64.
The bounds are first shown to hold for the float32 restatement itself, the comparator is shown to refuse a lost and a doubled slot, the
inputs are asserted to hold what they promise, and the argument checks of the two functions run before any device work.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import _lib
from dicp_amd.group import group_points, interpolate_features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import group_ref as gr  # noqa: E402
import hostbuild  # noqa: E402

DTYPES = [np.float32, np.float64]
SFX = {np.float32: "f32", np.float64: "f64"}
KS = (1, 3, 8, 32)
CS = (1, 33)
N_Q, M_ROWS, ROWS = 120, 257, 200


@pytest.fixture(scope="module")
def check():
    lib = hostbuild.build("group_check.cpp", "group_check", ("-Wall",))
    for fn in [lib.gc_live64, lib.gc_live32] + [getattr(lib, "gc_%s_%s" % (a, s)) for a in ("group", "interp", "gd2") for s in ("f32", "f64")]:
        fn.restype = None
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _table(m, C, dtype, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random((m, C)) * 2 - 1) * 10.0 ** rng.integers(-2, 3, size=(m, C))).astype(dtype)


def test_index_inputs_hold_every_kind_of_slot():
    for k in KS:
        for it in (np.int64, np.int32):
            idx = gr.make_idx(N_Q, k, M_ROWS, ROWS, 7 + k, it)
            assert idx.dtype == it
            kinds = gr.idx_kinds(idx, M_ROWS, ROWS)
            assert all(kinds.values()), (k, kinds)


@pytest.mark.parametrize("it", [np.int64, np.int32])
def test_liveness(check, it):
    """fails without dicp_group.h"""
    for rows in (0, 1, ROWS, M_ROWS):
        idx = gr.make_idx(N_Q, 8, M_ROWS, rows, 3, it)
        edge = np.array([[-1, 0, rows - 1, rows, rows + 1, np.iinfo(it).max, np.iinfo(it).min, -2]], dtype=it)
        idx = np.concatenate([idx, edge])
        out = np.zeros(idx.shape, dtype=np.uint8)
        (check.gc_live64 if it == np.int64 else check.gc_live32)(_ptr(idx), rows, ctypes.c_longlong(idx.size), _ptr(out))
        assert np.array_equal(out.astype(bool), gr.live_slots(idx, M_ROWS, rows))


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_matches_reference(check, dtype):
    for k in KS:
        for C in CS + (4,):
            idx = gr.make_idx(N_Q, k, M_ROWS, ROWS, 11 * k + C)
            f = _table(M_ROWS, C, dtype, k + C)
            for Cc in (0, 1, min(3, C), C):
                cen = _table(N_Q, Cc, dtype, 5) if Cc else None
                out = np.empty((N_Q, k, C), dtype=dtype)
                getattr(check, "gc_group_" + SFX[dtype])(_ptr(f), _ptr(idx), ROWS, _ptr(cen), Cc, N_Q, k, C, _ptr(out))
                assert gr.same_bits(out, gr.group_ref(f, idx, ROWS, cen)), (k, C, Cc)


def _interp_case(dtype, k, C, seed, near=False):
    idx = gr.make_idx(N_Q, k, M_ROWS, ROWS, seed)
    d2 = gr.make_d2(N_Q, k, seed + 1, dtype, near=near)
    f = _table(M_ROWS, C, dtype, seed + 2)
    g = _table(N_Q, C, dtype, seed + 3)
    return f, idx, d2, g


def _header_interp(check, f, idx, d2, eps, g):
    n, k = idx.shape
    C = f.shape[1]
    out, gd2 = np.empty((n, C), dtype=f.dtype), np.empty((n, k), dtype=f.dtype)
    sfx = SFX[f.dtype.type]
    getattr(check, "gc_interp_" + sfx)(_ptr(f), _ptr(idx), _ptr(d2), ctypes.c_double(eps), ROWS, n, k, C, _ptr(out))
    getattr(check, "gc_gd2_" + sfx)(_ptr(f), _ptr(idx), _ptr(d2), ctypes.c_double(eps), _ptr(g), _ptr(out), ROWS, n, k, C, _ptr(gd2))
    return out, gd2


def _ratio(got, exact, scale, factor):
    """the largest |got - exact| / (factor * scale); entries with a zero scale must be exact"""
    err = np.abs(got.astype(np.float64) - exact)
    assert (err[scale == 0] == 0).all()
    on = scale > 0
    return float((err[on] / (factor * scale[on])).max()) if on.any() else 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_interpolation_within_its_bounds(check, dtype):
    """The float32 / float64 restatement itself stays inside both bounds (forward: at most 0.30 of it), then the header is held to them.

    Measured on the restatement over k in {1, 3, 8, 32}, C in {1, 33}, d2 over eight decades with exact zeros: the forward's largest
    error / bound is 0.242 in float32 (0.076 in float64) and the d2 gradient's 0.197 (0.075) with the constant C + 3k + 16 as derived:
    no widening needed."""
    eps = 1e-8
    worst_f = worst_g = 0.0
    for k in KS:
        for C in CS:
            f, idx, d2, g = _interp_case(dtype, k, C, 100 * k + C)
            assert (d2 == 0).any() and (k == 1 or ((d2 == 0).sum(1) >= 2).any()) and np.isinf(d2).any()
            ex, sc = gr.interp_exact(f, idx, d2, eps, ROWS)
            gex, gsc = gr.gd2_exact(f, idx, d2, eps, g, ROWS)
            fb, gb = gr.interp_bound(k, dtype), gr.gd2_bound(k, C, dtype)
            rf = _ratio(gr.interp_ref(f, idx, d2, eps, ROWS), ex, sc, fb)
            rg = _ratio(gr.gd2_ref(f, idx, d2, eps, g, ROWS), gex, gsc, gb)
            worst_f, worst_g = max(worst_f, rf), max(worst_g, rg)
            assert rf <= 0.30 and rg <= 1.0, (k, C, rf, rg)
            out, gd2 = _header_interp(check, f, idx, d2, eps, g)
            assert _ratio(out, ex, sc, fb) <= 1.0 and _ratio(gd2, gex, gsc, gb) <= 1.0, (k, C)
            live = gr.live_slots(idx, M_ROWS, ROWS) & np.isfinite(d2)
            assert (gd2[~live] == 0).all() and (out[~live.any(1)] == 0).all()
    print("restatement: forward %.3f of its bound, g_d2 %.3f" % (worst_f, worst_g))


@pytest.mark.parametrize("dtype", DTYPES)
def test_comparator_refuses_a_lost_and_a_doubled_slot(dtype):
    """With live d2 within a factor of 4 of each other, a reference that drops one live slot of a query, or counts one twice, is outside
    the bound for that query: what the forward's comparison is there to catch."""
    eps = 1e-8
    for k in (3, 8, 32):
        f, idx, d2, _ = _interp_case(dtype, k, 33, 300 + k, near=True)
        live = gr.live_slots(idx, M_ROWS, ROWS)
        two = live.sum(1) >= 2
        assert two.sum() >= 10
        first = live.argmax(1)
        good = gr.interp_ref(f, idx, d2, eps, ROWS)
        ex, sc = gr.interp_exact(f, idx, d2, eps, ROWS)
        bound = gr.interp_bound(k, dtype) * sc
        assert (np.abs(good.astype(np.float64) - ex) <= bound).all()
        lost = idx.copy()
        lost[np.arange(N_Q), first] = -1
        twice_i = np.concatenate([idx, idx[np.arange(N_Q), first][:, None]], 1)
        twice_d = np.concatenate([d2, d2[np.arange(N_Q), first][:, None]], 1)
        for bad in (gr.interp_ref(f, lost, d2, eps, ROWS), gr.interp_ref(f, twice_i, twice_d, eps, ROWS)):
            off = (np.abs(bad.astype(np.float64) - ex) > bound).any(1)
            assert off[two].all()


def test_entry_points_reject_bad_arguments():
    """null pointers, a bad dtype, shapes, the index-width flag: refused before any launch (no GPU touched)"""
    _lib.build()
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    # dicp_group_forward(dtype, features, idx, idx64, rows, centers, Cc, N, n, m, k, C, out, stream)
    good = [0, one, one, 1, None, None, 0, 1, 10, 20, 4, 3, one, None]

    def call(fn, good, **kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return fn(*a)
    fwd = lib.dicp_group_forward
    assert call(fwd, good, a1=None) == 1 and call(fwd, good, a2=None) == 1 and call(fwd, good, a12=None) == 1 and call(fwd, good, a6=2) == 1
    assert call(fwd, good, a0=7) == 3 and call(fwd, good, a3=2) == 4
    assert [call(fwd, good, **{a: 0}) for a in ("a7", "a8", "a9", "a10", "a11")] == [2] * 5
    big = 2 ** 31 - 1
    assert call(fwd, good, a7=big, a8=big) == 2 and call(fwd, good, a7=big, a9=big, a11=big) == 2 and call(fwd, good, a8=big, a10=32, a11=big) == 2   # products past 2^62
    assert call(fwd, good, a10=33) == 2 and call(fwd, good, a5=one, a6=4) == 2 and call(fwd, good, a12=ctypes.c_void_p(258)) == 5
    # dicp_group_backward(dtype, grad_out, idx, idx64, rows, Cc, N, n, m, k, C, grad_features, grad_centers, stream)
    good = [0, one, one, 1, None, 0, 1, 10, 20, 4, 3, one, None, None]
    bwd = lib.dicp_group_backward
    assert call(bwd, good, a1=None) == 1 and call(bwd, good, a11=None) == 1 and call(bwd, good, a0=2) == 3 and call(bwd, good, a3=-1) == 4
    assert call(bwd, good, a9=0) == 2 and call(bwd, good, a12=one) == 2 and call(bwd, good, a5=4) == 2
    # dicp_interpolate_forward(dtype, features, idx, idx64, rows, d2, eps, N, n, m, k, C, out, stream)
    good = [0, one, one, 1, None, one, 1e-8, 1, 10, 20, 3, 1, one, None]
    jf = lib.dicp_interpolate_forward
    assert call(jf, good, a5=None) == 1 and call(jf, good, a12=None) == 1 and call(jf, good, a0=9) == 3 and call(jf, good, a3=5) == 4
    assert call(jf, good, a6=0.0) == 2 and call(jf, good, a6=float("nan")) == 2 and call(jf, good, a6=float("inf")) == 2 and call(jf, good, a10=0) == 2
    # dicp_interpolate_backward(dtype, grad_out, features, out, idx, idx64, rows, d2, eps, N, n, m, k, C, grad_features, grad_d2, stream)
    good = [0, one, one, one, one, 1, None, one, 1e-8, 1, 10, 20, 3, 1, one, one, None]
    jb = lib.dicp_interpolate_backward
    assert call(jb, good, a3=None) == 1 and call(jb, good, a14=None, a15=None) == 1 and call(jb, good, a0=9) == 3 and call(jb, good, a5=2) == 4
    assert call(jb, good, a8=-1.0) == 2 and call(jb, good, a13=0) == 2 and call(jb, good, a15=ctypes.c_void_p(258)) == 5


# ------------------------------------------------------------------ argument checks (raise before any device work)
F, I = torch.zeros(20, 4), torch.zeros(10, 3, dtype=torch.int64)
OPS = {"group_points": lambda f, i, **kw: group_points(f, i, **kw),
       "interpolate_features": lambda f, i, **kw: interpolate_features(f, i, _d2_like(f, i), **kw)}


def _d2_like(f, i):
    first = f[0] if isinstance(f, (list, tuple)) and f else f
    dt = first.dtype if isinstance(first, torch.Tensor) and first.dtype.is_floating_point else torch.float32
    if isinstance(i, (list, tuple)):
        return [torch.zeros(x.shape, dtype=dt) if isinstance(x, torch.Tensor) else x for x in i]
    return torch.zeros(i.shape, dtype=dt) if isinstance(i, torch.Tensor) else i


@pytest.mark.parametrize("op", sorted(OPS))
def test_bad_features_and_indices_raise(op):
    fn = OPS[op]
    bad = [(torch.zeros(20, 0), I),                                                  # C = 0
           (F, torch.zeros(10, 0, dtype=torch.int64)), (F, torch.zeros(10, 33, dtype=torch.int64)),       # k = 0, k = 33
           (F, torch.zeros(10, 3)), (F, torch.zeros(10, 3, dtype=torch.int16)), (F, torch.zeros(10, 3, dtype=torch.bool)),   # idx of a float / another dtype
           (F.to(torch.float16), I), (F.long(), I), ("abc", I), (F, np.zeros((10, 3), dtype=np.int64)),
           (F, torch.zeros(2, 10, 3, dtype=torch.int64)), (torch.zeros(2, 20, 4), I), ([F], I), (F, [I]),   # mismatched forms
           (torch.zeros(2, 20, 4), torch.zeros(3, 10, 3, dtype=torch.int64)), ([F, F], [I]),                # mismatched cloud counts
           ([F, torch.zeros(5, 3)], [I, I]), ([F, F], [I, torch.zeros(10, 4, dtype=torch.int64)]), ([F, F.double()], [I, I]),
           (torch.zeros(0, 4), I), (F, torch.zeros(0, 3, dtype=torch.int64)), ([], []), (F, torch.zeros(10, dtype=torch.int64))]
    for f, i in bad:
        with pytest.raises(ValueError):
            fn(f, i)
    with pytest.raises(ValueError):
        fn([F], [I], rows=[20])                                                      # rows on a list
    with pytest.raises(ValueError):
        fn(F, I, rows=[20])                                                          # rows need a padded batch
    for rows in ([21, 3], [-1, 3], [1.0, 2.0], [3]):
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 20, 4), torch.zeros(2, 10, 3, dtype=torch.int64), rows=rows)


def test_bad_centers_raise():
    for cen in (torch.zeros(10, 5), torch.zeros(10, 0), torch.zeros(9, 3), torch.zeros(10, 3, dtype=torch.float64), torch.zeros(1, 10, 3), [torch.zeros(10, 3)],
                torch.zeros(10, 3, dtype=torch.int64), "abc"):
        with pytest.raises(ValueError):
            group_points(F, I, centers=cen)
    with pytest.raises(ValueError):
        group_points([F, F], [I, I], centers=[torch.zeros(10, 3), torch.zeros(9, 3)])
    with pytest.raises(ValueError):
        group_points(torch.zeros(2, 20, 4), torch.zeros(2, 10, 3, dtype=torch.int64), centers=torch.zeros(3, 10, 3))


@pytest.mark.parametrize("eps", [0.0, -1e-8, float("nan"), float("inf"), 1e-60, 1e60, None, "1e-8", True, 10 ** 400])
def test_bad_eps_raises(eps):
    """(1e-60 and 1e60 are 0 and inf in float32)"""
    with pytest.raises(ValueError):
        interpolate_features(F, I, torch.zeros(10, 3), eps=eps)


def test_bad_d2_raises():
    for d2 in (torch.zeros(10, 3, dtype=torch.float64), torch.zeros(10, 4), torch.zeros(9, 3), torch.zeros(1, 10, 3), [torch.zeros(10, 3)], I, None):
        with pytest.raises(ValueError):
            interpolate_features(F, I, d2)


def test_valid_arguments_pass_the_checks():
    """what the refusals above leave through reaches the device (and, without one, its error): C = 1, k = 1 and 32, int32, every form"""
    calls = [lambda: group_points(torch.zeros(20, 1), torch.zeros(10, 1, dtype=torch.int32), centers=torch.zeros(10, 1)),
             lambda: group_points(torch.zeros(2, 20, 4), torch.zeros(2, 10, 32, dtype=torch.int64), rows=torch.tensor([20, 0])),
             lambda: interpolate_features([F, torch.zeros(5, 4)], [I, torch.zeros(7, 3, dtype=torch.int64)], [torch.zeros(10, 3), torch.zeros(7, 3)], eps=1e-6)]
    for c in calls:
        if torch.cuda.is_available():
            c()
        else:
            with pytest.raises(RuntimeError, match="no HIP device"):
                c()
