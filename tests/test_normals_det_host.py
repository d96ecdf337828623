"""CPU checks of the deterministic gradient of estimate_normals (deterministic=True) that need no GPU.

The rules of ``dicp_amd/csrc/dicp_normals_det.h`` -- the lines the HIP kernel runs -- are compiled with g++ through
tests/hostcheck/normals_det_check.cpp, run in a serial loop and held to the numpy restatement tests/normals_det_ref.py bit for bit, in
float32 and float64, with int32 and int64 neighbours, for lists of 0, 1, 63, 64, 65, 127, 128, 129 and 700 entries, rows at or past the
row count, 3 and 6 columns.  The comparison is shown to refuse six deliberately wrong restatements; the restatement itself lies within
the bound derived from the rule of the exact sum of its terms; garbage offsets / slots leave every access inside the arrays; and the
argument checks of the two entry points and of the Python front run before any device work.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import _lib
from dicp_amd.group import DET_CHUNK
from dicp_amd.normals import REC, estimate_normals

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import group_ref as gr  # noqa: E402
import hostbuild  # noqa: E402
import inverse_ref as ir  # noqa: E402
import normals_det_ref as nr  # noqa: E402

DTYPES = [np.float32, np.float64]
SFX = {np.float32: "f32", np.float64: "f64"}
D = DET_CHUNK
M, K, ROWS = 700, 8, 690
DEGREES = {3: 1, 5: D - 1, 7: D, 9: D + 1, 11: 2 * D - 1, 13: 2 * D, 15: 2 * D + 1, 17: 700, 695: 5}   # row 695 is past the row count; the other rows: 0
NAMED = [j for j in DEGREES if j < ROWS]


@pytest.fixture(scope="module")
def check():
    lib = hostbuild.build("normals_det_check.cpp", "normals_det_check", ("-Wall",))
    for s in SFX.values():
        fn = getattr(lib, "nd_det_" + s)
        fn.restype = None
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3
    lib.nd_record.restype = None
    lib.nd_record.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int]
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _case(idx_dtype=np.int64, seed=5):
    return nr.make_case(M, K, ROWS, DEGREES, seed, idx_dtype)


def _header(check, a, dtype, c=3, offsets=None, slots=None, out=None):
    rec, nbr = np.ascontiguousarray(a["rec"]), np.ascontiguousarray(a["nbr"])
    m, k = nbr.shape
    out = np.full((m, c), np.nan, dtype=dtype) if out is None else out
    off = a["offsets"] if offsets is None else offsets
    sl = a["slots"] if slots is None else slots
    getattr(check, "nd_det_" + SFX[dtype])(_ptr(rec), _ptr(nbr), int(nbr.dtype == np.int64), m, k, int(a["rows"]), c, _ptr(off), _ptr(sl), _ptr(out))
    return out


def test_constants(check):
    assert check.nd_chunk() == D == nr.DET_CHUNK and check.nd_rec() == REC == nr.REC == 13


def test_inputs_hold_what_they_promise():
    a = _case()
    deg = np.diff(a["offsets"])
    assert {j: int(deg[j]) for j in DEGREES} == {**DEGREES, 695: 0} and int(deg.sum()) == sum(DEGREES.values()) - 5
    assert sorted(set(deg.tolist())) == [0, 1, D - 1, D, D + 1, 2 * D - 1, 2 * D, 2 * D + 1, 700]
    assert (a["nbr"] == 695).sum() == 5 and (ir.slot_rows(a["nbr"], M, ROWS) != 695).all()         # named, past the count: not live
    f = a["rec"][:, 12]
    assert 0.15 < (f == 0).mean() < 0.25 and ((f == 0) | ((f >= 2 / 32) & (f <= 2 / 3))).all()
    iq = a["inf_query"]
    assert f[iq] == 0 and np.isinf(a["rec"][iq, 1]) and (ir.slot_rows(a["nbr"], M, ROWS)[iq] >= 0).any()
    for j in NAMED[1:]:                                     # every longer list holds entries without a term
        assert (ir.slot_rows(a["nbr"], M, ROWS)[f == 0] == j).any(), j


def test_record(check):
    """nrm_det_record: G6, mu, p, f = 2 / k_eff in their places; a query that contributes nothing keeps p alone"""
    G6, mu, p = np.arange(1.0, 7.0), np.arange(7.0, 10.0), np.arange(10.0, 13.0)
    R = np.full(REC, np.nan)
    check.nd_record(_ptr(R), 1, _ptr(G6), _ptr(mu), _ptr(p), 7)
    assert gr.same_bits(R, np.concatenate([G6, mu, p, [2.0 / 7]]))
    R[:] = np.nan
    check.nd_record(_ptr(R), 0, _ptr(G6), _ptr(mu), _ptr(p), 7)
    assert gr.same_bits(R, np.concatenate([np.zeros(9), p, [0.0]]))


@pytest.mark.parametrize("idx_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("c", [3, 6])
@pytest.mark.parametrize("dtype", DTYPES)
def test_header_matches_reference(check, dtype, c, idx_dtype):
    """fails without dicp_normals_det.h: bit for bit; every element stored (the output starts as NaN); rows nobody names, rows past the
    count and columns 3.. exactly +0; no NaN from the f = 0 query with an inf in its record"""
    a = _case(idx_dtype)
    ref = nr.ref_of(a, dtype, c=c)
    assert gr.same_bits(ref, nr.ref_of(a, dtype, c=c, fast=False))
    assert gr.same_bits(_header(check, a, dtype, c), ref)
    assert np.isfinite(ref).all() and (ref[NAMED, :3] != 0).all()
    zero = np.ones(M, dtype=bool)
    zero[NAMED] = False
    assert (ref[zero] == 0).all() and not np.signbit(ref[zero]).any() and (ref[:, 3:] == 0).all() and not np.signbit(ref[:, 3:]).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_comparison_refuses_wrong_restatements(dtype):
    """descending list order, a lost entry, a term for an f = 0 entry, mu left out, the chunk boundary off by one, the sum kept in a
    wider type, a wrong chunk size: each differs from the definition on the inputs of this file, so a kernel that made the same mistake
    would be refused"""
    a = _case()
    good = nr.ref_of(a, dtype)
    assert gr.same_bits(good, nr.ref_of(a, dtype))
    for w in nr.WRONG:
        assert not gr.same_bits(nr.ref_of(a, dtype, wrong=w), good), w
    assert np.isnan(nr.ref_of(a, dtype, wrong="term_for_f0")).any() and np.isfinite(good).all()
    short = [3, 5]                                          # lists that no chunk boundary touches either way
    assert gr.same_bits(nr.ref_of(a, dtype, wrong="chunk_off_by_one")[short], good[short])
    for Dw in (D // 2, 2 * D):
        bad = nr.ref_of(a, dtype, D=Dw)
        assert not gr.same_bits(bad, good) and gr.same_bits(bad[[3]], good[[3]])


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_within_the_derived_bound(dtype):
    """the restatement against the exact sum of its float64 terms: (deg + 2) u_T sum |t|, derived in normals_det_ref.normals_det_bound
    from the chunk rule and the rounding of a term -- no literal tolerance"""
    a = _case()
    a["rec"][a["inf_query"], 1] = 1.0
    S, A, deg, M = nr.normals_det_bound(a["rec"], a["nbr"], a["rows"], a["offsets"], a["slots"], dtype)
    assert deg.max() == 700
    err = np.abs(nr.ref_of(a, dtype)[:, :3].astype(np.longdouble) - S)
    B = (deg + 2)[:, None] * nr.U[dtype] * A
    assert (err <= B).all() and (err[NAMED] > 0).any() and (M >= A * (1 - 2.0 ** -40)).all()


def test_garbage_index_stays_in_range(check):
    """offsets / slots that are negative, huge, non-monotone, or name slots of other rows: every array sits between guard regions -- NaN
    around the records, a pattern around the output -- the output holds no NaN that a read outside would bring, the guards are
    unchanged, and the values are the restatement's on the same garbage"""
    m, k, rows = 40, 8, 35
    a = nr.make_case(m, k, rows, {2: 3, 4: 70, 6: 130, 37: 4}, 9)
    a["rec"][a["inf_query"], 1] = 1.0                       # (finite inputs: a NaN in the output can only come from outside)
    G = 4096

    def guarded(t, fill):
        buf = np.full(t.size + 2 * G, fill, dtype=t.dtype)
        buf[G:-G] = t.reshape(-1)
        return buf, buf[G:-G].reshape(t.shape)
    _, a["rec"] = guarded(a["rec"], np.nan)
    _, a["nbr"] = guarded(a["nbr"], 3)
    obuf, out = guarded(np.zeros((m, 3), dtype=np.float32), 12345.0)
    rng = np.random.default_rng(91)
    big = [-1, -2 ** 31, 2 ** 31 - 1, m * k, m * k + 1, -5, 10 ** 9]
    for trial in range(6):
        off = rng.choice(big + list(range(m * k)), size=m + 1).astype(np.int32)               # any order: hi < lo among them
        sl = rng.choice(big + list(range(m * k)), size=m * k).astype(np.int32)
        if trial == 0:
            off, sl = a["offsets"].copy(), rng.permutation(a["slots"]).astype(np.int32)       # valid lists, entries naming other rows
        out[:] = 7
        _header(check, a, np.float32, offsets=off, slots=sl, out=out)
        assert (obuf[:G] == 12345.0).all() and (obuf[-G:] == 12345.0).all()
        assert not np.isnan(out).any()
        assert gr.same_bits(out, nr.normals_det_ref(a["rec"], a["nbr"], rows, off, sl, np.float32)), trial


# ------------------------------------------------------------------ the entry points' status codes
NULL, SHAPE, DTYPE, ENUM, ALIGN = 1, 2, 3, 4, 5
F32, F64 = _lib.F32, _lib.F64


def P(addr):
    return ctypes.c_void_p(addr)


OK = P(4096)


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _bad_call(fn, good):
    def f(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        assert a != good, "a valid call would launch"
        return fn(*a)
    return f


def test_normals_backward_records_codes(lib):
    # (dtype, grid, g_normals, g_curvature, viewpoint, vp_per_cloud, rows, N, m, k, c, fwd_workspace, fwd_workspace_bytes, records, nbr_o, stream)
    for grid in (0, 1):
        need = (lib.dicp_normals_grid_workspace_bytes if grid else lib.dicp_normals_workspace_bytes)(F32, 2, 70, 8, 3, 0)
        assert need > 0
        f = _bad_call(lib.dicp_normals_backward_records, [F32, grid, OK, OK, None, 0, None, 2, 70, 8, 3, OK, need, OK, OK, None])
        for i in (11, 13, 14):
            assert f(**{"a%d" % i: None}) == NULL, i
        assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE and f(a1=2 + grid) == ENUM
        for i in (7, 8):
            assert f(**{"a%d" % i: 0}) == SHAPE, i
        assert f(a9=2) == SHAPE and f(a9=33) == SHAPE and f(a10=2) == SHAPE and f(a5=2) == SHAPE
        assert f(a12=need - 1) == SHAPE and f(a12=0) == SHAPE                                       # the forward's workspace, in full
        assert f(a9=16) == SHAPE                                                                    # (a larger k needs a larger one)
        assert f(a11=P(4096 + 128)) == ALIGN and f(a13=P(4096 + 4)) == ALIGN and f(a14=P(4096 + 2)) == ALIGN
        for i in (2, 3, 4):
            assert f(**{"a%d" % i: P(4096 + 2)}) == ALIGN and f(a0=F64, a12=1 << 30, **{"a%d" % i: P(4096 + 4)}) == ALIGN, i
        assert f(a6=P(4096 + 2)) == ALIGN
        assert f(a11=None, a0=2) == NULL and f(a0=2, a7=0) == DTYPE and f(a9=33, a13=P(4100)) == SHAPE
        assert f(a2=None, a13=P(4100)) == ALIGN and f(a3=None, a13=P(4100)) == ALIGN                # (either cotangent is optional)


def test_normals_gather_det_codes(lib):
    # (dtype, records, idx, idx64, rows, N, m, k, c, offsets, slots, grad_pts, stream)
    f = _bad_call(lib.dicp_normals_gather_det, [F32, OK, OK, 0, None, 2, 70, 8, 3, OK, OK, OK, None])
    for i in (1, 2, 9, 10, 11):
        assert f(**{"a%d" % i: None}) == NULL, i
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE and f(a3=2) == ENUM
    for i in (5, 6, 7):
        assert f(**{"a%d" % i: 0}) == SHAPE, i
    assert f(a7=33) == SHAPE and f(a8=2) == SHAPE
    assert f(a6=1 << 26, a7=32) == SHAPE and f(a6=(1 << 26) - 1, a7=32, a1=P(4100)) == ALIGN         # m k = 2^31; 2^31 - 32 passes
    assert f(a1=P(4096 + 4)) == ALIGN                                                               # the records are doubles
    for i in (2, 4, 9, 10, 11):
        assert f(**{"a%d" % i: P(4096 + 2)}) == ALIGN, i
    assert f(a0=F64, a11=P(4096 + 4)) == ALIGN and f(a3=1, a2=P(4096 + 4)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a5=0) == DTYPE and f(a7=33, a1=P(4100)) == SHAPE
    assert f(a4=OK, a1=P(4100)) == ALIGN                    # (rows is optional)


# ------------------------------------------------------------------ the Python front
X = torch.zeros(20, 3)


def _ops():
    return [lambda **kw: estimate_normals(X, k=3, **kw), lambda **kw: estimate_normals(X, k=3, method="grid", **kw),
            lambda **kw: estimate_normals([X, X], k=3, **kw), lambda **kw: estimate_normals(X[None], k=3, rows=torch.tensor([7]), **kw)]


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
