"""CPU checks of descriptor matching (dicp_amd/match.py) that need no GPU.

The rules of ``dicp_amd/csrc/dicp_match.h`` -- the lines the HIP kernels run -- are compiled with g++ through
tests/hostcheck/match_check.cpp (fma = __builtin_fmaf / __builtin_fma), run in a serial loop and held bit for bit to the numpy restatement
tests/match_ref.py: h, the score chain, the candidate rule, the (score, index) list, the refined d2, and both gradients with the
deterministic order of summation.  The float32 fma of the restatement is held to libm's; the comparison is shown to refuse deliberately
wrong restatements; the argument checks of the three Python functions and of the three entry points run before any device work; and the
end-to-end input of the GPU test is shown, on the restatement alone, to have exactly the ground truth as its answer.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import _lib
from dicp_amd.match import align_correspondences, knn_features, match_features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hostbuild  # noqa: E402
import match_cases as mc  # noqa: E402
import match_ref as mr  # noqa: E402

DTYPES = [np.float32, np.float64]
SFX = {np.float32: "f32", np.float64: "f64"}
P, I = ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def check():
    lib = hostbuild.build("match_check.cpp", "match_check", ("-Wall",))
    for s in SFX.values():
        getattr(lib, "mc_knn_" + s).restype = None
        getattr(lib, "mc_knn_" + s).argtypes = [P, I, I, P, I, I, I, I, P, P, P, P, P]
        getattr(lib, "mc_grads_" + s).restype = None
        getattr(lib, "mc_grads_" + s).argtypes = [P, P, P, I, P, I, I, I, I, P, P, P, P]
    lib.mc_fmaf.restype, lib.mc_fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    return lib


def _ptr(a):
    return a.ctypes.data_as(P)


def same_bits(a, b):
    """equal bit for bit (signed zeros told apart), NaN in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a).astype(a.dtype).view(u), np.where(nb, 0, b).astype(a.dtype).view(u)))


def header_knn(check, x, y, k, x_rows=None, y_rows=None):
    n, D = x.shape
    m = y.shape[0]
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    h, s_all = np.empty(m, x.dtype), np.empty((n, m), x.dtype)
    d2, idx, sc = np.empty((n, k), x.dtype), np.empty((n, k), np.int64), np.empty((n, k), x.dtype)
    getattr(check, "mc_knn_" + SFX[x.dtype.type])(_ptr(x), n, n if x_rows is None else x_rows, _ptr(y), m, m if y_rows is None else y_rows, D, k,
                                                 _ptr(h), _ptr(s_all), _ptr(d2), _ptr(idx), _ptr(sc))
    return h, s_all, d2, idx, sc


def cancelling(rng, n, m, D, dtype):
    """x close to y rows, scaled so that the partial sums of the score chain change sign: every fused product matters"""
    y = (rng.standard_normal((m, D)) * np.exp(rng.uniform(-3, 3, (m, 1)))).astype(dtype)
    x = (y[rng.integers(0, m, n)] * (1 + 1e-3 * rng.standard_normal((n, D)))).astype(dtype)
    return x, y


def test_fma32_is_libm_fmaf(check):
    rng = np.random.default_rng(1)
    a = rng.standard_normal(4000).astype(np.float32) * np.float32(2.0) ** rng.integers(-60, 60, 4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    with np.errstate(all="ignore"):
        p = (a.astype(np.float64) * b).astype(np.float32)
        cs = [rng.standard_normal(4000).astype(np.float32), -p, np.nextafter(-p, np.float32(np.inf)), np.nextafter(-p, np.float32(-np.inf)),
              (-p * np.float32(2.0) ** 24).astype(np.float32), (-p * np.float32(2.0) ** -24).astype(np.float32), np.full(4000, 1e-45, np.float32)]
    for c in cs:
        got = mr.fma32(a, b, c)
        want = np.array([check.mc_fmaf(float(u), float(v), float(w)) for u, v, w in zip(a, b, c)], dtype=np.float32)
        assert same_bits(got, want)
    with np.errstate(all="ignore"):
        assert not same_bits(mr.fma32(a, b, cs[2]), (a * b + cs[2]).astype(np.float32))             # a separate product is refused


CASES = [  # n, m, D, k, x_rows, y_rows
    (1, 1, 1, 1, None, None), (5, 3, 2, 4, None, None), (7, 40, 3, 5, None, None), (9, 33, 31, 8, 7, 30), (6, 65, 33, 17, None, 64),
    (4, 20, 64, 32, 4, 0), (3, 70, 256, 2, 0, None), (8, 12, 5, 16, None, None),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_header_matches_restatement(check, dtype, case):
    n, m, D, k, xr, yr = case
    if dtype == np.float64 and n * m * D > 20000:
        n, m = min(n, 3), min(m, 20)                        # (the float64 restatement is exact rational arithmetic per element)
        xr, yr = (None if xr is None else min(xr, n)), (None if yr is None else min(yr, m))
    rng = np.random.default_rng(n * 1000 + m + D)
    x, y = cancelling(rng, n, m, D, dtype)
    if m >= 12:
        y[5] = y[2]; y[11] = y[2]                           # exact duplicates: ties of the score
        y[7, 0] = np.nan; y[8, D - 1] = np.inf              # rows with no finite score
        x[0] = y[2]                                         # a query equal to a row: d2 = 0
    if n >= 4:
        x[3, D // 2] = -np.inf                              # a query with no neighbours
    h, s_all, d2, idx, sc = header_knn(check, x, y, k, xr, yr)
    assert same_bits(h, mr.half_norm(y))
    assert same_bits(s_all, mr.scores(x, y))
    rd2, ridx, rsc = mr.knn_features_ref(x, y, k, xr, yr, return_scores=True)
    assert np.array_equal(idx, ridx) and same_bits(d2, rd2)
    live = ridx >= 0
    assert same_bits(sc[live], rsc[live]) and np.all(np.isinf(d2[~live]))
    yr_ = m if yr is None else yr
    assert idx.max() < max(yr_, 0) or yr_ == 0 and idx.max() == -1
    if m >= 12 and (xr is None or xr > 0) and yr_ >= 12:
        assert d2[0, 0] == 0 and idx[0, 0] == 2
        if k >= 4:
            assert list(idx[0, :3]) == [2, 5, 11]           # duplicates in index order
        assert not np.isin(idx, (7, 8)).any()
    if n >= 4:
        assert np.all(idx[3] == -1)


def test_wrong_restatements_are_refused(check):
    rng = np.random.default_rng(3)
    x, y = cancelling(rng, 12, 48, 37, np.float32)
    y[20] = y[4]
    x[1] = y[4] * np.float32(1.001)
    h, s_all, d2, idx, sc = header_knn(check, x, y, 4)
    assert same_bits(s_all, mr.scores(x, y)) and np.array_equal(idx, mr.knn_features_ref(x, y, 4)[1])
    for wrong in ("unfused", "descending", "h_last"):
        assert not same_bits(s_all, mr.scores(x, y, wrong)), wrong
    assert not np.array_equal(idx, mr.knn_features_ref(x, y, 4, wrong="tie_high")[1])
    assert not same_bits(d2, mr.knn_features_ref(x, y, 4, wrong="d2_from_score")[0])
    assert same_bits(d2, mr.knn_features_ref(x, y, 4)[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients_and_their_order(check, dtype):
    rng = np.random.default_rng(4)
    n, m, D, k, rows = 150, 9, 5, 4, 8
    x = rng.standard_normal((n, D)).astype(dtype)
    y = rng.standard_normal((m, D)).astype(dtype)
    idx = rng.integers(0, 3, (n, k)).astype(np.int64)       # hubs: rows 0..2 are named about 150 times each, three chunks of 64
    idx[:, 3] = rng.integers(-1, m, n)                      # empty slots, a row past the count (8), rows named a few times
    idx[5] = 4                                              # one query names a row in all its slots
    g = rng.standard_normal((n, k)).astype(dtype)
    g[rng.random((n, k)) < 0.1] = 0
    off, slots = mr.invert(idx, m, rows)
    gx, gy = np.empty_like(x), np.empty_like(y)
    getattr(check, "mc_grads_" + SFX[dtype])(_ptr(g), _ptr(idx), _ptr(x), n, _ptr(y), m, rows, D, k, _ptr(off), _ptr(slots), _ptr(gx), _ptr(gy))
    idx_live = np.where(idx < rows, idx, -1)
    assert same_bits(gx, mr.grad_x_ref(g, idx, x, y))
    assert same_bits(gy, mr.grad_y_det_ref(g, idx, x, y, rows))
    assert not same_bits(gy, mr.grad_y_det_ref(g, idx, x, y, rows, wrong="descending"))
    assert not same_bits(gy, mr.grad_y_det_ref(g, idx, x, y, rows, wrong="one_chunk"))
    assert np.all(gy[rows:] == 0) and not np.signbit(gy[rows:]).any()
    exact = np.zeros((m, D))
    for i in range(n):
        for s in range(k):
            if idx_live[i, s] >= 0:
                exact[idx_live[i, s]] -= 2.0 * float(g[i, s]) * (x[i].astype(np.float64) - y[idx_live[i, s]])
    assert np.allclose(gy, exact, rtol=0, atol=1e-3 if dtype == np.float32 else 1e-11)


def test_end_to_end_input_has_the_ground_truth_as_its_answer():
    a = mc.end_to_end(seed=0)
    idx, d2 = mr.match_features_ref(a["fx"], a["fy"], mutual=True, ratio=0.8)
    assert np.array_equal(idx, a["gt"])
    assert 380 <= (a["gt"] >= 0).sum() <= 420 and np.all(np.isinf(d2[a["gt"] < 0]))
    only_mutual, _ = mr.match_features_ref(a["fx"], a["fy"], mutual=True, ratio=None)
    assert (only_mutual[a["gt"] < 0] >= 0).any()            # why the ratio is part of the test


# ------------------------------------------------------------------ the Python fronts: ValueError before any device work
def _bad(fn, *args, **kw):
    with pytest.raises(ValueError):
        fn(*args, **kw)


def test_argument_checks_of_the_python_functions():
    fx, fy = torch.zeros(5, 8), torch.zeros(7, 8)
    for k in (0, 33, 1.0, True, None):
        _bad(knn_features, fx, fy, k=k)
    _bad(knn_features, fx, torch.zeros(7, 9))
    _bad(knn_features, torch.zeros(5, 257), torch.zeros(7, 257))
    _bad(knn_features, fx, fy.double())
    _bad(knn_features, fx, fy[None])
    _bad(knn_features, fx.half(), fy.half())
    _bad(knn_features, fx, fy, deterministic=1)
    _bad(knn_features, fx, fy, _form="fast")
    _bad(knn_features, fx.double(), fy.double(), _form="mfma")
    _bad(knn_features, fx[None], fy[None], x_rows=torch.tensor([6]))
    _bad(knn_features, [fx], [fy], x_rows=torch.tensor([5]))
    for kw in (dict(mutual=1), dict(ratio=0.0), dict(ratio=1.5), dict(ratio="0.8"), dict(ratio=True), dict(max_d2=-1.0), dict(max_d2=float("nan")),
               dict(deterministic=None)):
        _bad(match_features, fx, fy, **kw)
    _bad(match_features, fx, torch.zeros(7, 9))
    x, y, idx = torch.zeros(5, 3), torch.zeros(7, 3), torch.zeros(5, dtype=torch.int64)
    _bad(align_correspondences, x, y, idx.float())
    _bad(align_correspondences, x, y, idx[:4])
    _bad(align_correspondences, x, y, idx + 7)
    _bad(align_correspondences, x, y, idx, weight=torch.ones(5, dtype=torch.float64))
    _bad(align_correspondences, x, y, idx, weight=torch.ones(4))
    _bad(align_correspondences, x[:, :2], y, idx)
    _bad(align_correspondences, [x], [y], idx)
    _bad(align_correspondences, x, y, idx, x_rows=torch.tensor([3]))
    _bad(align_correspondences, x[None], y[None], idx[None], x_rows=torch.tensor([6]))


# ------------------------------------------------------------------ the entry points' status codes (as tests/test_operator_entry_codes.py)
NULL, SHAPE, DTYPE, ENUM, ALIGN = 1, 2, 3, 4, 5
F32, F64 = _lib.F32, _lib.F64
BIG = 1 << 62
OK = P(4096)


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def entry(fn, good):
    def call(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        assert a != list(good), "a valid call would launch"
        return fn(*a)
    return call


def all_equal(call, positions, value, code, **kw):
    got = {i: call(**dict(kw, **{"a%d" % i: value})) for i in positions}
    assert got == {i: code for i in positions}


def test_knn_features_entry(lib):
    # (dtype, x, x_rows, n, y, y_rows, m, D, N, k, form, d2, idx, workspace, workspace_bytes, stream)
    need = lib.dicp_knn_features_workspace_bytes(F32, 2, 70)
    assert need == 768 and lib.dicp_knn_features_workspace_bytes(F64, 2, 70) == 1280
    f = entry(lib.dicp_knn_features, [F32, OK, None, 100, OK, None, 70, 32, 2, 8, 0, OK, OK, OK, need, None])
    all_equal(f, (1, 4, 11, 12, 13), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a10=3) == ENUM and f(a10=-1) == ENUM and f(a10=2, a0=F64, a14=BIG) == ENUM
    assert f(a7=0) == SHAPE and f(a7=257) == SHAPE and f(a9=0) == SHAPE and f(a9=33) == SHAPE
    assert f(a3=0) == SHAPE and f(a6=0) == SHAPE and f(a8=0) == SHAPE
    assert f(a7=256, a11=P(4098)) == ALIGN and f(a7=1, a11=P(4098)) == ALIGN and f(a9=32, a11=P(4098)) == ALIGN and f(a9=1, a11=P(4098)) == ALIGN
    assert f(a14=need - 1) == SHAPE and f(a14=need, a11=P(4098)) == ALIGN
    all_equal(f, (1, 4, 11), P(4096 + 2), ALIGN)
    all_equal(f, (1, 4, 11), P(4096 + 4), ALIGN, a0=F64, a14=BIG)
    all_equal(f, (2, 5), P(4096 + 2), ALIGN)
    assert f(a12=P(4096 + 4)) == ALIGN and f(a13=P(4096 + 8)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a7=0) == DTYPE and f(a7=0, a11=P(4098)) == SHAPE
    assert lib.dicp_knn_features_workspace_bytes(2, 2, 70) == 0 and lib.dicp_knn_features_workspace_bytes(F32, 0, 70) == 0


def test_knn_features_backward_entry(lib):
    # (dtype, g_d2, idx, x, y, n, m, D, N, k, grad_x, grad_y, stream)
    f = entry(lib.dicp_knn_features_backward, [F32, OK, OK, OK, OK, 100, 70, 32, 2, 8, OK, OK, None])
    all_equal(f, (1, 2, 3, 4), None, NULL)
    assert f(a0=2) == DTYPE
    assert f(a7=0) == SHAPE and f(a7=257) == SHAPE and f(a9=0) == SHAPE and f(a9=33) == SHAPE and f(a5=0) == SHAPE and f(a6=0) == SHAPE and f(a8=0) == SHAPE
    all_equal(f, (1, 3, 4, 10, 11), P(4096 + 2), ALIGN)
    all_equal(f, (1, 3, 4, 10, 11), P(4096 + 4), ALIGN, a0=F64)
    assert f(a2=P(4096 + 4)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a7=0) == DTYPE and f(a7=0, a1=P(4098)) == SHAPE
    assert f(a10=None, a11=None) == 0                       # nothing asked for: nothing launched


def test_knn_features_backward_det_entry(lib):
    # (dtype, g_d2, idx, y_rows, x, y, n, m, D, N, k, offsets, slots, grad_y, stream)
    f = entry(lib.dicp_knn_features_backward_det, [F32, OK, OK, None, OK, OK, 100, 70, 32, 2, 8, OK, OK, OK, None])
    all_equal(f, (1, 2, 4, 5, 11, 12, 13), None, NULL)
    assert f(a0=2) == DTYPE
    assert f(a8=0) == SHAPE and f(a8=257) == SHAPE and f(a10=0) == SHAPE and f(a10=33) == SHAPE and f(a6=0) == SHAPE and f(a7=0) == SHAPE and f(a9=0) == SHAPE
    assert f(a6=1 << 27, a10=32) == SHAPE                   # a cloud's slot numbers are int32
    all_equal(f, (1, 4, 5, 13), P(4096 + 2), ALIGN)
    all_equal(f, (1, 4, 5, 13), P(4096 + 4), ALIGN, a0=F64)
    all_equal(f, (3, 11, 12), P(4096 + 2), ALIGN)
    assert f(a2=P(4096 + 4)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a8=0) == DTYPE and f(a8=0, a1=P(4098)) == SHAPE
