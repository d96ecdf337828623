"""CPU checks of soft_match_features (dicp_amd/match.py) that need no GPU.

The rules of ``dicp_amd/csrc/dicp_softmatch.h`` -- the lines the HIP kernels run -- are compiled with g++ through
tests/hostcheck/softmatch_check.cpp, run in a serial loop in the vector kernels' order, and held to the float64 reference of
tests/softmatch_ref.py within its error model, in both dtypes; idx is held to match_ref.knn_features_ref(k=1) index for index.  A numpy
emulation of the kernels' order (both forward forms) proves the model; the comparator is shown to refuse deliberately wrong variants; the
argument checks of the Python function and of the entry points run before any device work.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import _lib
from dicp_amd.match import soft_match_features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hostbuild  # noqa: E402
import match_ref as mr  # noqa: E402
import softmatch_ref as sr  # noqa: E402

DTYPES = [np.float32, np.float64]
SFX = {np.float32: "f32", np.float64: "f64"}
P, I = ctypes.c_void_p, ctypes.c_int
GRADS = ("gfx", "gfy", "gvalues")


@pytest.fixture(scope="module")
def check():
    lib = hostbuild.build("softmatch_check.cpp", "softmatch_check", ("-Wall",))
    for s in SFX.values():
        getattr(lib, "sc_forward_" + s).restype = None
        getattr(lib, "sc_forward_" + s).argtypes = [P, I, I, P, I, I, I, P, I, ctypes.c_double, P, P, P, P]
        getattr(lib, "sc_backward_" + s).restype = None
        getattr(lib, "sc_backward_" + s).argtypes = [P, I, I, P, I, I, I, P, I, ctypes.c_double, P, P, P, P, P, P]
    return lib


def _ptr(a):
    return a.ctypes.data_as(P)


def header(check, fx, fy, values, tau, x_rows=None, y_rows=None, cot=None):
    n, D = fx.shape
    m, C = fy.shape[0], values.shape[1]
    dt = fx.dtype
    xr, yr = n if x_rows is None else x_rows, m if y_rows is None else y_rows
    out, lse, idx, prob = np.empty((n, C), dt), np.empty(n, dt), np.empty(n, np.int64), np.empty(n, dt)
    getattr(check, "sc_forward_" + SFX[dt.type])(_ptr(fx), n, xr, _ptr(fy), m, yr, D, _ptr(values), C, float(tau), _ptr(out), _ptr(lse), _ptr(idx), _ptr(prob))
    res = {"out": out, "lse": lse, "idx": idx, "prob": prob}
    if cot is not None:
        gx, gy, gv = np.empty_like(fx), np.empty_like(fy), np.empty_like(values)
        getattr(check, "sc_backward_" + SFX[dt.type])(_ptr(fx), n, xr, _ptr(fy), m, yr, D, _ptr(values), C, float(tau), _ptr(out), _ptr(lse), _ptr(cot),
                                                      _ptr(gx), _ptr(gy), _ptr(gv))
        res.update(gfx=gx, gfy=gy, gvalues=gv)
    return res


def held(res):
    return all(v[0] for v in res.values()), {k: round(v[1], 4) for k, v in res.items()}


CASES = [  # n, m, D, C, tau, x_rows, y_rows
    (1, 1, 1, 1, 1.0, None, None), (5, 17, 3, 3, 0.1, None, None), (9, 33, 31, 6, 0.01, 7, 30), (6, 65, 33, 8, 10.0, None, 64),
    (4, 20, 64, 3, 1.0, 4, 0), (3, 40, 8, 1, 0.1, 0, None), (33, 48, 5, 3, 0.01, None, None),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_header_within_the_bound(check, dtype, case):
    n, m, D, C, tau, xr, yr = case
    fx, fy, values, cot = sr.random_case(n, m, D, C, dtype, seed=n * 1000 + m + D)
    if m >= 17:
        fy[5] = fy[2]                                       # a tie of the score: idx is the lowest index
        fy[7, 0] = np.nan; fy[8, D - 1] = np.inf            # rows with no finite score
        fx[0] = fy[2]
    if n >= 4:
        fx[3, D // 2] = -np.inf                             # a query without a candidate
    if yr is not None:
        fy[yr:] = 1e30; values[yr:] = np.nan                # pad rows hold garbage
    if xr is not None:
        fx[xr:] = np.nan; cot[xr:] = np.nan
    got = header(check, fx, fy, values, tau, xr, yr, cot)
    ok, worst = held(sr.hold(got, fx, fy, values, tau, xr, yr, cot))
    assert ok, worst
    assert np.array_equal(got["idx"], mr.knn_features_ref(fx, fy, 1, xr, yr)[1][:, 0])
    dead = got["idx"] < 0
    assert np.all(got["out"][dead] == 0) and np.all(got["prob"][dead] == 0) and np.all(got["gfx"][dead] == 0)
    if n >= 4 and (xr is None or xr > 3):
        assert got["idx"][3] == -1
    if yr is not None:
        assert np.all(got["gfy"][yr:] == 0) and np.all(got["gvalues"][yr:] == 0)
    for k in GRADS:
        assert np.isfinite(got[k]).all(), k


@pytest.mark.parametrize("form", ["valu", "mfma"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_emulation_within_the_bound(dtype, form):
    for (n, m, D, C, tau, seed) in ((7, 70, 5, 3, 0.01, 1), (5, 129, 16, 6, 1.0, 2), (4, 33, 3, 8, 10.0, 3)):
        fx, fy, values, cot = sr.random_case(n, m, D, C, dtype, seed)
        got = sr.emulate(fx, fy, values, tau, cot=cot, form=form)
        ok, worst = held(sr.hold(got, fx, fy, values, tau, cot=cot, form=form))
        assert ok, (n, m, worst)
    # descending scores: the maximum rises at every block
    fx, fy, values, cot = sr.random_case(3, 100, 2, 3, dtype, 4)
    fy[:, 0], fy[:, 1], fx[:] = np.linspace(3.0, 1.0, 100), 0.0, 0.0
    fx[:, 0] = 1.0
    got = sr.emulate(fx, fy, values, 0.05, cot=cot, form=form)
    ok, worst = held(sr.hold(got, fx, fy, values, 0.05, cot=cot, form=form))
    assert ok, worst


def test_header_and_emulation_agree(check):
    """the g++ build walks the emulation's order: the same results up to the library functions (exp, log, 1 / S) the two call"""
    fx, fy, values, cot = sr.random_case(6, 50, 7, 3, np.float64, 9)
    a, b = header(check, fx, fy, values, 0.1, cot=cot), sr.emulate(fx, fy, values, 0.1, cot=cot)
    assert np.array_equal(a["idx"], b["idx"])
    for k in ("out", "prob") + GRADS:
        assert np.allclose(a[k], b[k], rtol=1e-13, atol=1e-300), k


def test_wrong_variants_are_refused():
    n, m, D, C, tau = 6, 80, 4, 3, 0.02
    fx, fy, values, cot = sr.random_case(n, m, D, C, np.float32, 11)
    # every query's best row is late (row 70): an early block carries weight that a missing rescale leaves too heavy
    fy[70] = 0.05                                           # (its logit is not 0: an lse without its maximum shows)
    fx[:] = 0.01 * fx
    fy[15] = 0.06                                           # the row a skipped tile edge loses carries weight
    yr = 75
    fx[2] = fy[yr - 1]                                      # query 2: all its mass on the last live row, where 16 u_T on 1 / S shows
    fy[yr:] = fx[0]; values[yr:] = 5.0                      # pad rows that would take the mass if they were let in
    good = sr.emulate(fx, fy, values, tau, y_rows=yr, cot=cot)
    ok, worst = held(sr.hold(good, fx, fy, values, tau, y_rows=yr, cot=cot))
    assert ok, worst
    for fault in sr.FAULTS:
        bad = sr.emulate(fx, fy, values, tau, y_rows=yr, cot=cot, fault=fault, at=2)
        ok, worst = held(sr.hold(bad, fx, fy, values, tau, y_rows=yr, cot=cot))
        assert not ok, (fault, worst)


def test_model_matches_the_sources():
    src = open(os.path.join(HERE, "..", "dicp_amd", "csrc", "dicp_softmatch.h")).read()
    hip = open(os.path.join(HERE, "..", "dicp_amd", "csrc", "softmatch.hip")).read()
    assert "constexpr int SOFT_ROWS = %d;" % sr.SOFT_ROWS in src
    assert "return __expf(v)" in src and "return __logf(v)" in src and "__builtin_amdgcn_rcpf(v)" in src
    assert "constexpr int SM_STAGE_TILES = %d;" % sr.SM_STAGE_TILES in hip and "constexpr int SM_STAGE_WORDS = %d;" % sr.SM_STAGE_WORDS in hip
    assert [sr.stage_rows(D) for D in (1, 32, 33, 64, 128, 255, 256)] == [256, 256, 224, 128, 64, 32, 32]


# ------------------------------------------------------------------ the Python front: ValueError before any device work
def _bad(*args, **kw):
    with pytest.raises(ValueError):
        soft_match_features(*args, **kw)


def test_argument_checks_of_the_python_function():
    fx, fy, v = torch.zeros(5, 8), torch.zeros(7, 8), torch.zeros(7, 3)
    for t in (0, 0.0, -1.0, True, float("nan"), float("inf"), torch.tensor(0.1), "0.1", None, 1e-60):
        _bad(fx, fy, v, t)
    _bad(fx, fy, torch.zeros(7, 0), 0.1)
    _bad(fx, fy, torch.zeros(7, 9), 0.1)
    _bad(fx, fy, torch.zeros(6, 3), 0.1)
    _bad(fx, fy, v.double(), 0.1)
    _bad(fx, fy, v[None], 0.1)
    _bad(fx, fy, [v], 0.1)
    _bad([fx], [fy], v, 0.1)
    _bad([fx], [fy], [torch.zeros(6, 3)], 0.1)
    _bad(fx, torch.zeros(7, 9), v, 0.1)
    _bad(fx, fy.double(), v, 0.1)
    _bad(fx, fy[None], v, 0.1)
    _bad(torch.zeros(5, 257), torch.zeros(7, 257), v, 0.1)
    _bad(fx[None], fy[None], v[None], 0.1, x_rows=torch.tensor([6]))
    _bad(fx, fy, v, 0.1, return_best=1)
    _bad(fx, fy, v, 0.1, _form="fast")
    _bad(fx.double(), fy.double(), v.double(), 0.1, _form="mfma")


# ------------------------------------------------------------------ the entry points' status codes (as tests/test_match_host.py)
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


def test_soft_match_entry(lib):
    # (dtype, x, x_rows, n, y, y_rows, m, D, N, values, C, tau, form, out, lse, idx, prob, workspace, workspace_bytes, stream)
    need = lib.dicp_soft_match_workspace_bytes(F32, 2, 70)
    assert need == 768 and lib.dicp_soft_match_workspace_bytes(F64, 2, 70) == 1280
    f = entry(lib.dicp_soft_match, [F32, OK, None, 100, OK, None, 70, 32, 2, OK, 3, 0.1, 0, OK, OK, OK, OK, OK, need, None])
    all_equal(f, (1, 4, 9, 13, 14, 15, 16, 17), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a12=3) == ENUM and f(a12=-1) == ENUM and f(a12=2, a0=F64, a18=BIG) == ENUM
    assert f(a7=0) == SHAPE and f(a7=257) == SHAPE and f(a10=0) == SHAPE and f(a10=9) == SHAPE
    assert f(a3=0) == SHAPE and f(a6=0) == SHAPE and f(a8=0) == SHAPE
    for tau in (0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60):
        assert f(a11=tau) == SHAPE, tau
    assert f(a11=1e-60, a0=F64, a18=BIG, a13=P(4098)) == ALIGN                          # (a finite scale in float64)
    assert f(a18=need - 1) == SHAPE and f(a18=need, a13=P(4098)) == ALIGN
    all_equal(f, (1, 4, 9, 13, 14, 16), P(4096 + 2), ALIGN)
    all_equal(f, (1, 4, 9, 13, 14, 16), P(4096 + 4), ALIGN, a0=F64, a18=BIG)
    all_equal(f, (2, 5), P(4096 + 2), ALIGN)
    assert f(a15=P(4096 + 4)) == ALIGN and f(a17=P(4096 + 8)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a7=0) == DTYPE and f(a7=0, a13=P(4098)) == SHAPE
    assert lib.dicp_soft_match_workspace_bytes(2, 2, 70) == 0 and lib.dicp_soft_match_workspace_bytes(F32, 0, 70) == 0


def test_soft_match_backward_entry(lib):
    # (dtype, x, x_rows, n, y, y_rows, m, D, N, values, C, tau, form, out, lse, grad_out, grad_x, grad_y, grad_values, workspace, workspace_bytes, stream)
    need = lib.dicp_soft_match_workspace_bytes(F32, 2, 70)
    f = entry(lib.dicp_soft_match_backward, [F32, OK, None, 100, OK, None, 70, 32, 2, OK, 3, 0.1, 0, OK, OK, OK, OK, OK, OK, OK, need, None])
    all_equal(f, (1, 4, 9, 13, 14, 15, 19), None, NULL)
    assert f(a0=2) == DTYPE
    assert f(a12=3) == ENUM and f(a12=-1) == ENUM and f(a12=2, a0=F64, a20=BIG) == ENUM and f(a12=2, a7=129) == ENUM
    assert f(a7=0) == SHAPE and f(a7=257) == SHAPE and f(a10=0) == SHAPE and f(a10=9) == SHAPE and f(a3=0) == SHAPE and f(a6=0) == SHAPE and f(a8=0) == SHAPE
    assert f(a11=0.0) == SHAPE and f(a11=float("nan")) == SHAPE and f(a20=need - 1) == SHAPE
    all_equal(f, (1, 4, 9, 13, 14, 15, 16, 17, 18), P(4096 + 2), ALIGN)
    all_equal(f, (1, 4, 9, 13, 14, 15, 16, 17, 18), P(4096 + 4), ALIGN, a0=F64, a20=BIG)
    all_equal(f, (2, 5), P(4096 + 2), ALIGN)
    assert f(a19=P(4096 + 8)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a7=0) == DTYPE and f(a7=0, a1=P(4098)) == SHAPE
    assert f(a16=None, a17=None, a18=None) == 0             # nothing asked for: nothing launched
