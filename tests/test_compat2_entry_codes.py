"""The status codes of the second-order compatibility entry points (include/dicp_hip.h: dicp_compat2_bits / _common / _rank / _seeds) for
every class of bad call, on a machine without a GPU: the checks run before any launch, in the order null (1), dtype (3), shape (2),
alignment (5).  As tests/test_compat_entry_codes.py: every call here is invalid, so nothing is launched.
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
N_MAX = 1 << 20


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


def test_geometry_and_limits(lib):
    v = [ctypes.c_int32() for _ in range(4)]
    lib.dicp_compat2_geometry(*[ctypes.byref(t) for t in v])
    rows, tile, words, chunk = [t.value for t in v]
    assert rows == 64 and tile % 64 == 0 and tile >= 64 and words >= 1 and chunk % rows == 0
    lib.dicp_compat2_geometry(None, None, None, None)           # any may be left out
    assert M.N2_MAX == N_MAX and (M.MEMBERS_MIN, M.MEMBERS_MAX) == (3, 32)
    assert lib.dicp_abi_version() == 11                         # the entry points are additive


def test_compat2_bits_entry(lib):
    # (dtype, pairs, P, N, n, threshold, min_length, adj, degree, degree2, stream)
    f = entry(lib.dicp_compat2_bits, [F32, OK, OK, 2, 100, 0.05, 0.0, OK, OK, OK, None])
    all_equal(f, (1, 2, 7, 8, 9), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a3=0) == SHAPE and f(a3=-1) == SHAPE and f(a4=0) == SHAPE and f(a4=N_MAX + 1) == SHAPE
    assert f(a3=1 << 20, a4=1 << 14) == SHAPE                   # the words: N n W >= 2^40
    assert f(a3=1 << 14, a4=N_MAX) == SHAPE                     # the grids
    assert f(a5=0.0) == SHAPE and f(a5=-1.0) == SHAPE and f(a5=NAN) == SHAPE and f(a5=INF) == SHAPE
    assert f(a6=-1e-9) == SHAPE and f(a6=NAN) == SHAPE and f(a6=INF) == SHAPE
    all_equal(f, (1,), P(4096 + 2), ALIGN)
    all_equal(f, (1,), P(4096 + 4), ALIGN, a0=F64)
    all_equal(f, (2, 8), P(4096 + 2), ALIGN)
    all_equal(f, (7, 9), P(4096 + 4), ALIGN)
    assert f(a1=None, a0=2) == NULL and f(a0=2, a4=0) == DTYPE and f(a4=0, a1=P(4098)) == SHAPE


def test_compat2_common_entry(lib):
    # (adj, P, N, n, degree2, stream)
    f = entry(lib.dicp_compat2_common, [OK, OK, 2, 100, OK, None])
    all_equal(f, (0, 1, 4), None, NULL)
    assert f(a2=0) == SHAPE and f(a3=0) == SHAPE and f(a3=N_MAX + 1) == SHAPE and f(a2=1 << 20, a3=1 << 14) == SHAPE
    all_equal(f, (0, 4), P(4096 + 4), ALIGN)
    all_equal(f, (1,), P(4096 + 2), ALIGN)
    assert f(a0=None, a3=0) == NULL and f(a3=0, a0=P(4100)) == SHAPE


def test_compat2_rank_entry(lib):
    # (dtype, degree2, P, N, n, seeds, rank2, score2, seedpos, stream)
    f = entry(lib.dicp_compat2_rank, [F32, OK, OK, 2, 100, 8, OK, OK, OK, None])
    all_equal(f, (1, 2, 6, 7), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a3=0) == SHAPE and f(a4=0) == SHAPE and f(a4=N_MAX + 1) == SHAPE and f(a3=1 << 20, a4=1 << 14) == SHAPE
    assert f(a5=-1) == SHAPE and f(a5=65537) == SHAPE
    assert f(a8=None) == SHAPE and f(a5=0) == SHAPE             # seedpos goes with seeds > 0, and only with it
    all_equal(f, (1,), P(4096 + 4), ALIGN)
    all_equal(f, (2, 6, 8), P(4096 + 2), ALIGN)
    all_equal(f, (7,), P(4096 + 2), ALIGN)
    all_equal(f, (7,), P(4096 + 4), ALIGN, a0=F64)
    assert f(a1=None, a0=2) == NULL and f(a0=2, a4=0) == DTYPE and f(a4=0, a1=P(4100)) == SHAPE


def test_compat2_seeds_entry(lib):
    # (dtype, pairs, P, adj, seedpos, N, n, seeds, members, member_list, poses, stream)
    f = entry(lib.dicp_compat2_seeds, [F32, OK, OK, OK, OK, 2, 100, 8, 16, OK, OK, None])
    all_equal(f, (1, 2, 3, 4, 9, 10), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a5=0) == SHAPE and f(a6=0) == SHAPE and f(a6=N_MAX + 1) == SHAPE and f(a5=1 << 20, a6=1 << 14) == SHAPE
    assert f(a7=0) == SHAPE and f(a7=65537) == SHAPE and f(a8=2) == SHAPE and f(a8=33) == SHAPE
    assert f(a5=1 << 16, a6=64, a7=1 << 15) == SHAPE            # the grid: N seeds >= 2^31
    all_equal(f, (1, 10), P(4096 + 2), ALIGN)
    all_equal(f, (1, 10), P(4096 + 4), ALIGN, a0=F64)
    all_equal(f, (2, 4, 9), P(4096 + 2), ALIGN)
    all_equal(f, (3,), P(4096 + 4), ALIGN)
    assert f(a1=None, a0=2) == NULL and f(a0=2, a8=2) == DTYPE and f(a8=2, a1=P(4098)) == SHAPE
