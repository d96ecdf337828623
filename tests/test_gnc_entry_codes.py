"""The status codes of dicp_gnc_fit (include/dicp_hip.h) for every class of bad call, on a machine without a GPU: the checks run before
any launch, in the order null (1), dtype (3), enum (4), shape (2), alignment (5).  As tests/test_iss_entry_codes.py: every call here is
invalid, so nothing is launched.
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


def test_the_abi_version_stays(lib):
    assert lib.dicp_abi_version() == 11 == _lib.ABI_VERSION
    assert "dicp_gnc_fit" in _lib.EXPORTS and (_lib.GNC_TLS, _lib.GNC_GM) == (0, 1)


def test_gnc_fit_entry(lib):
    # (dtype, pairs, P, u, N, n, loss, threshold, growth, iterations, weights_packed, rounds, status, mu, pose_last, trace, stream)
    f = entry(lib.dicp_gnc_fit, [F32, OK, OK, None, 2, 300, 0, 0.05, 1.4, 128, OK, OK, OK, OK, OK, None, None])
    got = {i: f(**{"a%d" % i: None}) for i in (1, 2, 10, 11, 12, 13, 14)}
    assert got == {i: NULL for i in got}
    assert f(a3=OK, a15=OK, a1=P(4098)) == ALIGN                                  # the user weights and the trace are optional
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a6=2) == ENUM and f(a6=-1) == ENUM
    assert f(a6=1, a1=P(4098)) == ALIGN
    assert f(a4=0) == SHAPE and f(a5=0) == SHAPE and f(a4=-3) == SHAPE and f(a5=(1 << 30) + 1) == SHAPE
    for t in (0.0, -0.05, NAN, INF, -INF, 1e-200, 1e200):
        assert f(a7=t) == SHAPE
    assert f(a7=1e-150, a1=P(4098)) == ALIGN and f(a7=1e150, a1=P(4098)) == ALIGN
    for g in (1.0, 0.5, -1.4, 16.000001, NAN, INF):
        assert f(a8=g) == SHAPE
    assert f(a8=16.0, a1=P(4098)) == ALIGN and f(a8=1.0000001, a1=P(4098)) == ALIGN
    for it in (0, -1, 257, 1 << 20):
        assert f(a9=it) == SHAPE
    assert f(a9=1, a1=P(4098)) == ALIGN and f(a9=256, a1=P(4098)) == ALIGN
    for i in (1, 10, 14):
        assert f(**{"a%d" % i: P(4096 + 2)}) == ALIGN and f(**{"a%d" % i: P(4096 + 4), "a0": F64}) == ALIGN
    assert f(a3=P(4096 + 2)) == ALIGN and f(a3=P(4096 + 4), a0=F64) == ALIGN
    for i in (2, 11, 12):
        assert f(**{"a%d" % i: P(4096 + 2)}) == ALIGN
    assert f(a13=P(4096 + 4)) == ALIGN and f(a15=P(4096 + 4)) == ALIGN          # mu and the trace are doubles in both dtypes
    # the order of the checks
    assert f(a1=None, a0=2) == NULL and f(a0=2, a6=5) == DTYPE and f(a6=5, a9=0) == ENUM and f(a9=0, a1=P(4098)) == SHAPE
