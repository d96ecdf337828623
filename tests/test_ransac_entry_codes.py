"""The status codes of the RANSAC entry points (include/dicp_hip.h: dicp_ransac_hypotheses / _score / _best, dicp_pair_residuals) for every
class of bad call, on a machine without a GPU: the checks run before any launch, in the order null (1), dtype (3), shape (2), alignment
(5).  As tests/test_operator_entry_codes.py: every call here is invalid, so nothing is launched.
"""
import ctypes

import pytest

from dicp_amd import _lib

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


def test_slice_is_a_whole_number_of_waves(lib):
    s = lib.dicp_ransac_slice()
    assert s >= 64 and s % 64 == 0


def test_ransac_hypotheses_entry(lib):
    # (dtype, pairs, P, N, n, H, seed, poses, samples, stream)
    f = entry(lib.dicp_ransac_hypotheses, [F32, OK, OK, 2, 100, 64, 7, OK, OK, None])
    all_equal(f, (1, 2, 7, 8), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a3=0) == SHAPE and f(a4=0) == SHAPE and f(a5=0) == SHAPE and f(a5=65537) == SHAPE and f(a4=(1 << 30) + 1) == SHAPE
    assert f(a3=1 << 20, a4=1 << 30, a5=65536) == SHAPE     # the score kernel's grid
    all_equal(f, (1, 7), P(4096 + 2), ALIGN)
    all_equal(f, (1, 7), P(4096 + 4), ALIGN, a0=F64)
    all_equal(f, (2, 8), P(4096 + 2), ALIGN)
    assert f(a1=None, a0=2) == NULL and f(a0=2, a5=0) == DTYPE and f(a5=0, a1=P(4098)) == SHAPE


def test_ransac_score_entry(lib):
    # (dtype, pairs, P, poses, N, n, H, threshold, counts, stream)
    f = entry(lib.dicp_ransac_score, [F32, OK, OK, OK, 2, 100, 64, 0.05, OK, None])
    all_equal(f, (1, 2, 3, 8), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a4=0) == SHAPE and f(a5=0) == SHAPE and f(a6=0) == SHAPE and f(a6=65537) == SHAPE
    all_equal(f, (7,), 0.0, SHAPE)
    assert f(a7=-1.0) == SHAPE and f(a7=NAN) == SHAPE and f(a7=INF) == SHAPE
    all_equal(f, (1, 3), P(4096 + 2), ALIGN)
    all_equal(f, (1, 3), P(4096 + 4), ALIGN, a0=F64)
    all_equal(f, (2, 8), P(4096 + 2), ALIGN)
    assert f(a1=None, a0=2) == NULL and f(a0=2, a7=0.0) == DTYPE and f(a7=0.0, a1=P(4098)) == SHAPE


def test_ransac_best_entry(lib):
    # (dtype, counts, poses, P, N, H, best, best_count, pose_best, stream)
    f = entry(lib.dicp_ransac_best, [F32, OK, OK, OK, 2, 64, OK, OK, OK, None])
    all_equal(f, (1, 2, 3, 6, 7, 8), None, NULL)
    assert f(a0=2) == DTYPE
    assert f(a4=0) == SHAPE and f(a5=0) == SHAPE and f(a5=65537) == SHAPE
    all_equal(f, (2, 8), P(4096 + 2), ALIGN)
    all_equal(f, (2, 8), P(4096 + 4), ALIGN, a0=F64)
    all_equal(f, (1, 3, 6, 7), P(4096 + 2), ALIGN)
    assert f(a1=None, a0=2) == NULL and f(a0=2, a5=0) == DTYPE and f(a5=0, a2=P(4098)) == SHAPE


def test_pair_residuals_entry(lib):
    # (dtype, x, y, idx, x_rows, pose, N, n, m, d2, stream)
    f = entry(lib.dicp_pair_residuals, [F32, OK, OK, OK, None, OK, 2, 100, 70, OK, None])
    all_equal(f, (1, 2, 3, 5, 9), None, NULL)
    assert f(a0=2) == DTYPE
    assert f(a6=0) == SHAPE and f(a7=0) == SHAPE and f(a8=0) == SHAPE and f(a7=(1 << 30) + 1) == SHAPE and f(a8=(1 << 30) + 1) == SHAPE
    all_equal(f, (1, 2, 5, 9), P(4096 + 2), ALIGN)
    all_equal(f, (1, 2, 5, 9), P(4096 + 4), ALIGN, a0=F64)
    all_equal(f, (3, 4), P(4096 + 2), ALIGN)
    assert f(a1=None, a0=2) == NULL and f(a0=2, a7=0) == DTYPE and f(a7=0, a1=P(4098)) == SHAPE
