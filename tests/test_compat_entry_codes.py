"""The status codes of the compatibility entry points (include/dicp_hip.h: dicp_compat_scores / _rank) for every class of bad call, on a
machine without a GPU: the checks run before any launch, in the order null (1), dtype (3), shape (2), alignment (5).  As
tests/test_ransac_entry_codes.py: every call here is invalid, so nothing is launched.
"""
import ctypes

import pytest

from dicp_amd import _lib
from dicp_amd import match as M

NULL, SHAPE, DTYPE, ENUM, ALIGN = 1, 2, 3, 4, 5
F32, F64 = _lib.F32, _lib.F64
P = ctypes.c_void_p
OK = P(4096)
NAN, INF = float("nan"), float("inf")


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


def test_geometry_is_whole_waves(lib):
    rows, tile = ctypes.c_int32(), ctypes.c_int32()
    lib.dicp_compat_geometry(ctypes.byref(rows), ctypes.byref(tile))
    assert rows.value >= 64 and rows.value % 64 == 0 and tile.value >= 64 and tile.value % 64 == 0
    lib.dicp_compat_geometry(None, None)                        # either may be left out
    assert M.ITER_MAX == 64


def test_compat_scores_entry(lib):
    # (dtype, pairs, P, N, n, iterations, threshold, min_length, w, wmax, score, degree, stream)
    f = entry(lib.dicp_compat_scores, [F32, OK, OK, 2, 100, 10, 0.05, 0.0, OK, OK, OK, OK, None])
    all_equal(f, (1, 2, 8, 9, 10, 11), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a3=0) == SHAPE and f(a3=-1) == SHAPE and f(a4=0) == SHAPE and f(a4=(1 << 30) + 1) == SHAPE
    assert f(a3=1 << 30, a4=1 << 20) == SHAPE                   # the grid
    assert f(a5=-1) == SHAPE and f(a5=65) == SHAPE
    assert f(a6=0.0) == SHAPE and f(a6=-1.0) == SHAPE and f(a6=NAN) == SHAPE and f(a6=INF) == SHAPE
    assert f(a7=-1e-9) == SHAPE and f(a7=NAN) == SHAPE and f(a7=INF) == SHAPE
    all_equal(f, (1, 8, 9, 10), P(4096 + 2), ALIGN)
    all_equal(f, (1, 8, 9, 10), P(4096 + 4), ALIGN, a0=F64)
    all_equal(f, (2, 11), P(4096 + 2), ALIGN)
    assert f(a1=None, a0=2) == NULL and f(a0=2, a5=65) == DTYPE and f(a5=65, a1=P(4098)) == SHAPE


def test_compat_rank_entry(lib):
    # (dtype, score, P, N, n, rank, stream)
    f = entry(lib.dicp_compat_rank, [F32, OK, OK, 2, 100, OK, None])
    all_equal(f, (1, 2, 5), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a3=0) == SHAPE and f(a4=0) == SHAPE and f(a4=(1 << 30) + 1) == SHAPE and f(a3=1 << 30, a4=1 << 20) == SHAPE
    all_equal(f, (1,), P(4096 + 2), ALIGN)
    all_equal(f, (1,), P(4096 + 4), ALIGN, a0=F64)
    all_equal(f, (2, 5), P(4096 + 2), ALIGN)
    assert f(a1=None, a0=2) == NULL and f(a0=2, a4=0) == DTYPE and f(a4=0, a1=P(4098)) == SHAPE
