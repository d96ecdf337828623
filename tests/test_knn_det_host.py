"""CPU checks of the deterministic y-gradient of knn_points / ball_query / chamfer_distance (deterministic=True) that need no GPU.

The rules of ``dicp_amd/csrc/dicp_knn_det.h`` -- the lines the HIP kernel runs -- are compiled with g++ through
tests/hostcheck/knn_det_check.cpp, run in a serial loop and held to the numpy restatement tests/knn_det_ref.py bit for bit, in float32 and
float64, for lists of 0, 1, 63, 64, 65, 128, 129 and 4097 entries, a query naming one row in two slots, rows at or past the row count and
3 and 6 columns, in the serial form, in the hub form and in the kernel's choice between them.  The comparison is shown to refuse five
deliberately wrong restatements; the restatement itself lies within a bound derived from the rule of the exact sum; garbage offsets /
slots leave every access inside the arrays; and the argument checks of the entry point and of the Python front run before any device
work.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import _lib
from dicp_amd.ball import ball_query
from dicp_amd.group import DET_CHUNK
from dicp_amd.knn import DET_HUB, chamfer_distance, knn_points

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import group_ref as gr  # noqa: E402
import hostbuild  # noqa: E402
import inverse_ref as ir  # noqa: E402
import knn_det_ref as kr  # noqa: E402
import walk_layouts as wl  # noqa: E402

DTYPES = [np.float32, np.float64]
SFX = {np.float32: "f32", np.float64: "f64"}
D = DET_CHUNK
N_Q, K, M, ROWS = 700, 8, 40, 36
DEGREES = {3: 1, 5: D - 1, 7: D, 9: D + 1, 11: 2 * D, 13: 2 * D + 1, 15: 4097, 38: 5}      # row 38 is past the row count; the other rows: 0


@pytest.fixture(scope="module")
def check():
    lib = hostbuild.build("knn_det_check.cpp", "knn_det_check", ("-Wall",))
    for s in SFX.values():
        fn = getattr(lib, "kd_det_" + s)
        fn.restype = None
        fn.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _case(dtype, cy=3, cx=3, seed=5):
    return kr.make_case(N_Q, K, M, ROWS, DEGREES, dtype, seed, cx=cx, cy=cy)


def _header(check, a, form=0, offsets=None, slots=None, out=None):
    g, idx, x, y = (np.ascontiguousarray(a[key]) for key in ("g", "idx", "x", "y"))
    n, k = idx.shape
    out = np.full(y.shape, np.nan, dtype=g.dtype) if out is None else out
    off = a["offsets"] if offsets is None else offsets
    sl = a["slots"] if slots is None else slots
    getattr(check, "kd_det_" + SFX[g.dtype.type])(form, _ptr(g), _ptr(idx), _ptr(x), x.shape[1], n, k, _ptr(y), y.shape[1], y.shape[0], int(a["rows"]),
                                                   _ptr(off), _ptr(sl), _ptr(out))
    return out


def test_constants(check):
    assert check.kd_chunk() == D and check.kd_hub() == DET_HUB >= 1


def test_inputs_hold_what_they_promise():
    a = _case(np.float32)
    deg = np.diff(a["offsets"])
    assert {j: int(deg[j]) for j in DEGREES} == {**DEGREES, 38: 0} and int(deg.sum()) == sum(DEGREES.values()) - 5
    assert sorted(set(deg.tolist())) == [0, 1, D - 1, D, D + 1, 2 * D, 2 * D + 1, 4097]
    row = ir.slot_rows(a["idx"], M, ROWS)
    srt = np.sort(row, axis=1)
    assert ((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any()                           # a query naming one row in two slots
    assert (a["idx"] == 38).sum() == 5 and (row != 38).all()                                  # named, past the count: not live
    live = row >= 0
    assert (a["g"][live] == 0).any() and not np.isfinite(a["g"][~live]).any() and np.isfinite(a["g"][live]).all()
    iq = a["inf_query"]
    assert live[iq].any() and (a["g"][iq][live[iq]] == 0).all() and np.isinf(a["x"][iq, 0])


@pytest.mark.parametrize("cy", [3, 6])
@pytest.mark.parametrize("dtype", DTYPES)
def test_header_matches_reference(check, dtype, cy):
    """fails without dicp_knn_det.h: bit for bit, the serial walk, the hub fold of every list of more than one chunk, and the kernel's
    choice; every element stored (the output starts as NaN); rows nobody names, rows past the count and columns 3.. exactly +0"""
    a = _case(dtype, cy=cy, cx=cy)
    ref = kr.ref_of(a)
    assert gr.same_bits(ref, kr.ref_of(a, fast=True))
    for form in (0, 1, 2):
        assert gr.same_bits(_header(check, a, form), ref), form
    assert np.isfinite(ref).all() and (ref[list(DEGREES)[:-1], :3] != 0).all()
    zero = np.ones(M, dtype=bool)
    zero[list(DEGREES)[:-1]] = False
    assert (ref[zero] == 0).all() and not np.signbit(ref[zero]).any() and (ref[:, 3:] == 0).all() and not np.signbit(ref[:, 3:]).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_comparison_refuses_wrong_restatements(dtype):
    """descending list order, a lost entry, the terms summed in a wider type and rounded at the end, the g == 0 skip removed while an
    inf coordinate sits behind a zero cotangent, the chunk boundary off by one, a wrong chunk size: each differs from the definition on
    the inputs of this file, so a kernel that made the same mistake would be refused"""
    a = _case(dtype)
    good = kr.ref_of(a)
    assert gr.same_bits(good, kr.ref_of(a))
    for w in kr.WRONG:
        assert not gr.same_bits(kr.ref_of(a, wrong=w), good), w
    assert np.isnan(kr.ref_of(a, wrong="no_zero_skip")).any() and np.isfinite(good).all()
    short = [3, 5]                                          # lists that no chunk boundary touches either way
    assert gr.same_bits(kr.ref_of(a, wrong="chunk_off_by_one")[short], good[short])
    for Dw in (D // 2, 2 * D):
        bad = kr.ref_of(a, D=Dw)
        assert not gr.same_bits(bad, good) and gr.same_bits(bad[[3]], good[[3]])


@pytest.mark.parametrize("cy", [3, 6])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_within_the_derived_bound(dtype, cy):
    """the restatement against the exact sum of the extended-precision terms: (min(deg, 64) + ceil(deg / 64) + 3) u sum |t|, derived
    in knn_det_ref.knn_det_bound from the chunk rule and the roundings of a term -- no literal tolerance"""
    a = _case(dtype, cy=cy, cx=cy)
    S, B, deg, _ = kr.knn_det_bound(a["g"], a["idx"], a["x"], a["y"], a["rows"], dtype)
    assert sorted(set(deg.tolist())) == [0, 1, D - 1, D, D + 1, 2 * D, 2 * D + 1, 4097]
    ratio = wl.assert_within(kr.ref_of(a)[:, :3], S, B, "knn_det_ref")
    assert 0 < ratio <= 1


def test_garbage_index_stays_in_range(check):
    """offsets / slots that are negative, huge, non-monotone, or name slots of other rows: every array sits between guard regions --
    NaN around the inputs, a pattern around the output -- the output holds no NaN that a read outside would bring, the guards are
    unchanged, and the values are the restatement's on the same garbage"""
    a = kr.make_case(40, 8, 30, 25, {2: 3, 4: 70, 6: 130, 27: 4}, np.float32, 9)
    a["x"][a["inf_query"], 0] = 1.0                          # (finite inputs: a NaN in the output can only come from outside)
    n, k, m = 40, 8, 30
    G = 4096

    def guarded(t, fill):
        buf = np.full(t.size + 2 * G, fill, dtype=t.dtype)
        buf[G:-G] = t.reshape(-1)
        return buf, buf[G:-G].reshape(t.shape)
    live = ir.slot_rows(a["idx"], m, 25) >= 0
    a["g"] = np.where(live, a["g"], 1.0).astype(np.float32)
    for key in ("g", "x", "y"):
        _, a[key] = guarded(a[key], np.nan)
    _, a["idx"] = guarded(a["idx"], 3)
    obuf, out = guarded(np.zeros((m, 3), dtype=np.float32), 12345.0)
    rng = np.random.default_rng(91)
    big = [-1, -2 ** 31, 2 ** 31 - 1, n * k, n * k + 1, -5, 10 ** 9]
    for trial in range(6):
        off = rng.choice(big + list(range(n * k)), size=m + 1).astype(np.int32)               # any order: hi < lo among them
        sl = rng.choice(big + list(range(n * k)), size=n * k).astype(np.int32)
        if trial == 0:
            off, sl = a["offsets"].copy(), rng.permutation(a["slots"]).astype(np.int32)       # valid lists, entries naming other rows
        for form in (0, 1, 2):
            out[:] = 7
            _header(check, a, form, offsets=off, slots=sl, out=out)
            assert (obuf[:G] == 12345.0).all() and (obuf[-G:] == 12345.0).all()
            assert not np.isnan(out).any()
            assert gr.same_bits(out, kr.knn_det_ref(a["g"], a["idx"], a["x"], a["y"], 25, off, sl)), (trial, form)


# ------------------------------------------------------------------ the entry point's status codes
NULL, SHAPE, DTYPE, ENUM, ALIGN = 1, 2, 3, 4, 5
F32, F64 = _lib.F32, _lib.F64


def P(addr):
    return ctypes.c_void_p(addr)


OK = P(4096)


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_knn_backward_y_det_codes(lib):
    # (dtype, g_d2, idx, y_rows, x, cx, n, y, cy, m, N, k, offsets, slots, grad_y, stream)
    good = [F32, OK, OK, None, OK, 3, 100, OK, 3, 70, 2, 8, OK, OK, OK, None]

    def f(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        assert a != good, "a valid call would launch"
        return lib.dicp_knn_backward_y_det(*a)
    for i in (1, 2, 4, 7, 12, 13, 14):
        assert f(**{"a%d" % i: None}) == NULL, i
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    for i in (6, 9, 10, 11):
        assert f(**{"a%d" % i: 0}) == SHAPE, i
    assert f(a11=33) == SHAPE and f(a5=2) == SHAPE and f(a8=2) == SHAPE
    assert f(a6=1 << 26, a11=32) == SHAPE and f(a6=(1 << 26) - 1, a11=32, a1=P(4098)) == ALIGN   # n k = 2^31; 2^31 - 32 passes
    for i in (1, 4, 7, 14, 3, 12, 13):
        assert f(**{"a%d" % i: P(4096 + 2)}) == ALIGN, i
    for i in (1, 4, 7, 14):
        assert f(a0=F64, **{"a%d" % i: P(4096 + 4)}) == ALIGN, i
    assert f(a2=P(4096 + 4)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a10=0) == DTYPE and f(a11=33, a1=P(4098)) == SHAPE
    assert f(a3=OK, a1=P(4098)) == ALIGN                    # (y_rows is optional)
    assert lib.dicp_abi_version() == _lib.ABI_VERSION == 11


# ------------------------------------------------------------------ the Python front
X, Y = torch.zeros(10, 3), torch.zeros(20, 3)


def _ops():
    return [lambda **kw: knn_points(X, Y, k=3, **kw), lambda **kw: knn_points(X, Y, k=3, method="grid", **kw), lambda **kw: ball_query(X, Y, 0.5, k=3, **kw),
            lambda **kw: chamfer_distance(X, Y, **kw), lambda **kw: chamfer_distance([X, X], [Y, Y], method="grid", **kw),
            lambda **kw: knn_points(X[None], Y[None], k=3, y_rows=torch.tensor([7]), **kw)]


def test_bad_deterministic_raises():
    """fails without the feature (a TypeError: no such keyword): anything but a bool is a ValueError before any device work"""
    for op in _ops():
        for det in ("yes", 1, 0, None, torch.tensor(True)):
            with pytest.raises(ValueError, match="deterministic must be True or False"):
                op(deterministic=det)


def test_valid_arguments_pass_the_checks():
    """what the refusal above leaves through reaches the device (and, without one, its error)"""
    for op in _ops():
        for det in (True, False):
            if torch.cuda.is_available():
                op(deterministic=det)
            else:
                with pytest.raises(RuntimeError, match="no HIP device"):
                    op(deterministic=det)
