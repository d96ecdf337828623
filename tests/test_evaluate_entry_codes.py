"""The status codes of dicp_evaluate_poses and dicp_evaluate_workspace_bytes (include/dicp_hip.h) for every class of bad call, on a
machine without a GPU: the checks run before any launch, in the order null (1), dtype (3), shape (2), alignment (5).  As
tests/test_gnc_entry_codes.py: every call here is invalid, so nothing is launched.
"""
import ctypes

import pytest

from dicp_amd import _lib

NULL, SHAPE, DTYPE, ALIGN = 1, 2, 3, 5
F32, F64 = _lib.F32, _lib.F64
P = ctypes.c_void_p
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


def test_the_abi_version_stays(lib):
    assert lib.dicp_abi_version() == 11 == _lib.ABI_VERSION
    assert "dicp_evaluate_poses" in _lib.EXPORTS and "dicp_evaluate_workspace_bytes" in _lib.EXPORTS


def test_workspace_bytes(lib):
    f = lib.dicp_evaluate_workspace_bytes                                           # (N, H, n)
    assert f(1, 1, 1) == 512 and f(1, 1, 256) == 512 and f(1, 1, 257) == 512        # 80 + 4 bytes per workgroup, each part rounded up to 256
    assert f(2, 3, 1000) == 2048 + 256 and f(32, 64, 16384) == 32 * 64 * 64 * 84
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1, 65537, 1), (1, 1, (1 << 30) + 1), (1 << 12, 1 << 12, 1 << 15)):
        assert f(*bad) == 0, bad
    assert f(1, 65536, 1) > 0 and f(1 << 11, 1 << 12, 1 << 15) > 0                  # 2^30 workgroups fit, 2^31 do not


def test_evaluate_poses_entry(lib):
    # (dtype, source, c, source_rows, n, poses, H, y_plans, y_keys, y_perm, y_rows4, m, N, workspace, workspace_bytes, sums, counts, fitness, rmse,
    #  idx, d2, stream)
    ws = lib.dicp_evaluate_workspace_bytes(2, 5, 300)
    f = entry(lib.dicp_evaluate_poses, [F32, OK, 3, None, 300, OK, 5, OK, OK, OK, OK, 700, 2, OK, ws, OK, OK, OK, OK, None, None, None])
    got = {i: f(**{"a%d" % i: None}) for i in (1, 5, 7, 8, 9, 10, 13, 15, 16, 17, 18)}
    assert got == {i: NULL for i in got}
    assert f(a3=OK, a19=OK, a20=OK, a1=P(4098)) == ALIGN                            # the row counts, idx and d2 are optional
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    for i, v in ((2, 2), (2, 0), (4, 0), (4, -1), (4, (1 << 30) + 1), (6, 0), (6, -2), (6, 65537), (11, 0), (11, (1 << 30) + 1), (12, 0), (12, -1),
                 (14, ws - 1), (14, 0)):
        assert f(**{"a%d" % i: v}) == SHAPE, (i, v)
    assert f(a12=1 << 20, a6=1 << 12) == SHAPE                                      # 2^20 x 2^12 x 2 workgroups do not fit one launch
    assert f(a6=1, a1=P(4098)) == ALIGN and f(a2=6, a1=P(4098)) == ALIGN and f(a14=ws + 1, a1=P(4098)) == ALIGN
    for i in (1, 5, 20):
        assert f(**{"a%d" % i: P(4096 + 2)}) == ALIGN and f(**{"a%d" % i: P(4096 + 4), "a0": F64}) == ALIGN
    assert f(a10=P(4096 + 8)) == ALIGN and f(a10=P(4096 + 16), a0=F64) == ALIGN     # the packed rows are vectors of four
    for i in (3, 9, 16):
        assert f(**{"a%d" % i: P(4096 + 2)}) == ALIGN
    for i in (7, 8, 15, 17, 18, 19):
        assert f(**{"a%d" % i: P(4096 + 4)}) == ALIGN
    assert f(a13=P(4096 + 128)) == ALIGN
    # the order of the checks
    assert f(a1=None, a0=2) == NULL and f(a0=2, a6=0) == DTYPE and f(a6=0, a1=P(4098)) == SHAPE
