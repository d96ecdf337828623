"""The status code of every class of bad call of the knn_points, normals and voxel entry points of libdicp_hip.so (include/dicp_hip.h).

CPU only: every call here is refused by the argument checks, before any launch, so no GPU is touched.  Per function one call per class of
refusal -- a null required pointer, a bad dtype, each bad shape or k bound, a workspace one byte too small, one misaligned pointer of each
alignment class -- with the exact code, and the order of the checks where two faults meet (null, then dtype, then shape, then alignment).
A call that shows a check PASSING carries a misaligned pointer as well, so that it ends with 5 instead of launching.
"""
import ctypes

import pytest

from dicp_amd import _lib

NULL, SHAPE, DTYPE, ALIGN = 1, 2, 3, 5          # DICP_ERR_NULL / _SHAPE / _DTYPE / _ALIGN
F32, F64 = _lib.F32, _lib.F64
BIG = 1 << 62                                   # a workspace size that is never too small


def P(addr):
    return ctypes.c_void_p(addr)


OK = P(4096)                                    # aligned for every class; never dereferenced: each call is refused first


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def entry(fn, good):
    """-> call(a3=..., a7=...): fn on the valid argument list `good` with the arguments at those positions replaced"""
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


def test_knn_points(lib):
    # (dtype, x_tgs4, x_perm, x_rows, n, y_keys, y_tgs4, y_perm, y_rows, m, N, k, d2, idx, workspace, workspace_bytes, walked, stream)
    need = lib.dicp_knn_points_workspace_bytes(F32, 2, 100, 70, 8, 0)
    assert need == 2 * 128 * 8 * 4
    f = entry(lib.dicp_knn_points, [F32, OK, OK, None, 100, OK, OK, OK, None, 70, 2, 8, OK, OK, OK, need, None, None])
    all_equal(f, (1, 2, 5, 6, 7, 12, 13, 14), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a10=0) == SHAPE and f(a4=0) == SHAPE and f(a9=0) == SHAPE and f(a11=0) == SHAPE and f(a11=33) == SHAPE
    assert f(a4=67108801, a15=BIG) == SHAPE and f(a4=67108800, a15=BIG, a12=P(4098)) == ALIGN        # padded n * 32 slots must fit an int
    assert f(a15=need - 1) == SHAPE and f(a15=need, a12=P(4098)) == ALIGN
    all_equal(f, (1, 6), P(4096 + 8), ALIGN)                                                 # 4 elements: 16 bytes in float32
    all_equal(f, (1, 6), P(4096 + 16), ALIGN, a0=F64, a15=BIG)                               # ... 32 in float64
    all_equal(f, (5, 12), P(4096 + 2), ALIGN)                                                # one element
    all_equal(f, (5, 12), P(4096 + 4), ALIGN, a0=F64, a15=BIG)
    all_equal(f, (2, 7, 14, 3, 8), P(4096 + 2), ALIGN)                                       # int32
    all_equal(f, (13, 16), P(4096 + 4), ALIGN)                                               # 64-bit
    assert f(a1=None, a0=2) == NULL and f(a0=2, a10=0) == DTYPE and f(a11=33, a12=P(4098)) == SHAPE
    assert lib.dicp_knn_points_workspace_bytes(2, 2, 100, 70, 8, 0) == 0 and lib.dicp_knn_points_workspace_bytes(F32, 2, 100, 70, 33, 0) == 0


def test_knn_points_backward(lib):
    # (dtype, g_d2, x_tgs4, x_perm, x_rows, n, cx, y_tgs4, y_perm, m, cy, N, k, fwd_workspace, grad_x, grad_y, workspace, workspace_bytes, stream)
    need = lib.dicp_knn_points_workspace_bytes(F32, 2, 100, 70, 8, 1)
    assert need == 2 * 128 * 3 * 4
    f = entry(lib.dicp_knn_points_backward, [F32, OK, OK, OK, None, 100, 3, OK, OK, 70, 3, 2, 8, OK, OK, OK, OK, need, None])
    all_equal(f, (1, 2, 3, 7, 8, 13), None, NULL)
    assert f(a16=None) == NULL                                                               # grad_y needs the workspace
    assert f(a0=2) == DTYPE
    assert f(a11=0) == SHAPE and f(a5=0) == SHAPE and f(a9=0) == SHAPE and f(a12=0) == SHAPE and f(a12=33) == SHAPE
    assert f(a6=2) == SHAPE and f(a10=2) == SHAPE
    assert f(a17=need - 1) == SHAPE and f(a17=need, a1=P(4098)) == ALIGN
    assert f(a17=0, a15=None, a16=None, a1=P(4098)) == ALIGN                                 # no grad_y: no workspace asked for
    all_equal(f, (2, 7), P(4096 + 8), ALIGN)
    all_equal(f, (2, 7), P(4096 + 16), ALIGN, a0=F64, a17=BIG)
    all_equal(f, (1, 14, 15), P(4096 + 2), ALIGN)
    all_equal(f, (1, 14, 15), P(4096 + 4), ALIGN, a0=F64, a17=BIG)
    all_equal(f, (3, 8, 13, 4), P(4096 + 2), ALIGN)
    assert f(a16=P(4096 + 8)) == ALIGN                                                       # the workspace: 16 bytes
    assert f(a1=None, a0=2) == NULL and f(a0=2, a11=0) == DTYPE and f(a6=2, a1=P(4098)) == SHAPE
    assert f(a14=None, a15=None) == 0                                                        # nothing asked for: nothing launched


def test_normals_forward(lib):
    # (dtype, pts, c, rows, N, m, k, viewpoint, vp_per_cloud, normals, curvature, neighbors, workspace, workspace_bytes, walked, stream)
    need = lib.dicp_normals_workspace_bytes(F32, 2, 100, 8, 3, 0)
    assert need > 0 and need % 256 == 0
    f = entry(lib.dicp_normals_forward, [F32, OK, 3, None, 2, 100, 8, OK, 1, OK, OK, OK, OK, need, None, None])
    all_equal(f, (1, 9, 12), None, NULL)
    assert f(a0=2) == DTYPE
    assert f(a4=0) == SHAPE and f(a5=0) == SHAPE and f(a6=2) == SHAPE and f(a6=33) == SHAPE and f(a8=2) == SHAPE and f(a8=-1) == SHAPE
    assert f(a2=2) == SHAPE and f(a5=67108801, a13=BIG) == SHAPE
    assert f(a13=need - 1) == SHAPE and f(a13=need, a1=P(4098)) == ALIGN
    assert f(a6=3, a1=P(4098)) == ALIGN and f(a6=32, a13=BIG, a1=P(4098)) == ALIGN          # the bounds of k themselves pass
    assert f(a12=P(4096 + 128)) == ALIGN                                                     # the workspace: 256 bytes
    all_equal(f, (1, 7, 9, 10), P(4096 + 2), ALIGN)
    all_equal(f, (1, 7, 9, 10), P(4096 + 4), ALIGN, a0=F64, a13=BIG)
    assert f(a11=P(4096 + 4)) == ALIGN                                                       # the int64 neighbour lists
    assert f(a1=None, a0=2) == NULL and f(a0=2, a4=0) == DTYPE and f(a6=2, a1=P(4098)) == SHAPE
    assert lib.dicp_normals_workspace_bytes(F32, 2, 100, 2, 3, 0) == 0 and lib.dicp_normals_workspace_bytes(F32, 2, 100, 8, 2, 0) == 0


def test_normals_backward(lib):
    # (dtype, g_normals, g_curvature, viewpoint, vp_per_cloud, rows, N, m, k, c, fwd_workspace, grad_pts, workspace, workspace_bytes, stream)
    need = lib.dicp_normals_workspace_bytes(F32, 2, 100, 8, 3, 1)
    assert need == 2 * 128 * 3 * 4
    f = entry(lib.dicp_normals_backward, [F32, OK, OK, OK, 1, None, 2, 100, 8, 3, OK, OK, OK, need, None])
    all_equal(f, (10, 11, 12), None, NULL)
    assert f(a0=2) == DTYPE
    assert f(a6=0) == SHAPE and f(a7=0) == SHAPE and f(a8=2) == SHAPE and f(a8=33) == SHAPE and f(a4=2) == SHAPE and f(a9=2) == SHAPE
    assert f(a13=need - 1) == SHAPE and f(a13=need, a11=P(4098)) == ALIGN
    assert f(a10=P(4096 + 128)) == ALIGN and f(a12=P(4096 + 8)) == ALIGN                     # 256 bytes; 16 bytes
    all_equal(f, (1, 2, 3, 11), P(4096 + 2), ALIGN)
    all_equal(f, (1, 2, 3, 11), P(4096 + 4), ALIGN, a0=F64, a13=BIG)
    assert f(a10=None, a0=2) == NULL and f(a0=2, a6=0) == DTYPE and f(a8=2, a11=P(4098)) == SHAPE


def test_voxel_count(lib):
    # (dtype, pts, c, rows, N, m, sx, sy, sz, origin, origin_per_cloud, min_points, rows_out, workspace, workspace_bytes, stream)
    need = lib.dicp_voxel_workspace_bytes(F32, 2, 100, 3)
    assert need > 0 and need % 256 == 0
    f = entry(lib.dicp_voxel_count, [F32, OK, 3, None, 2, 100, 0.5, 0.5, 0.5, OK, 1, 1, OK, OK, need, None])
    all_equal(f, (1, 12, 13), None, NULL)
    assert f(a0=2) == DTYPE
    assert f(a4=0) == SHAPE and f(a5=0) == SHAPE and f(a2=2) == SHAPE and f(a4=1 << 29, a14=BIG) == SHAPE
    assert f(a5=0x7fffffff - 4096, a14=BIG) == SHAPE and f(a5=0x7fffffff - 4097, a14=BIG, a1=P(4098)) == ALIGN   # m + a tile of 4096 rows fits an int
    assert f(a10=2) == SHAPE and f(a10=-1) == SHAPE and f(a11=0) == SHAPE
    for i in (6, 7, 8):
        all_equal(f, (i,), 0.0, SHAPE)
        all_equal(f, (i,), -1.0, SHAPE)
        all_equal(f, (i,), float("inf"), SHAPE)
        all_equal(f, (i,), float("nan"), SHAPE)
    assert f(a14=need - 1) == SHAPE and f(a14=need, a1=P(4098)) == ALIGN
    assert f(a13=P(4096 + 128)) == ALIGN
    all_equal(f, (1, 9), P(4096 + 2), ALIGN)
    all_equal(f, (1, 9), P(4096 + 4), ALIGN, a0=F64)
    all_equal(f, (12, 3), P(4096 + 2), ALIGN)
    assert f(a1=None, a0=2) == NULL and f(a0=2, a4=0) == DTYPE and f(a11=0, a1=P(4098)) == SHAPE
    assert lib.dicp_voxel_workspace_bytes(2, 2, 100, 3) == 0 and lib.dicp_voxel_workspace_bytes(F32, 2, 100, 2) == 0


def test_voxel_reduce(lib):
    # (dtype, pts, c, N, m, M, workspace, workspace_bytes, centroids, counts, inverse, stream)
    need = lib.dicp_voxel_workspace_bytes(F32, 2, 100, 3)
    f = entry(lib.dicp_voxel_reduce, [F32, OK, 3, 2, 100, 40, OK, need, OK, OK, OK, None])
    all_equal(f, (1, 6, 10, 8, 9), None, NULL)
    assert f(a5=0, a8=None, a9=None, a1=P(4098)) == ALIGN                                    # no voxels: no centroids / counts asked for
    assert f(a0=2) == DTYPE
    assert f(a3=0) == SHAPE and f(a4=0) == SHAPE and f(a2=2) == SHAPE and f(a5=-1) == SHAPE and f(a5=101) == SHAPE
    assert f(a5=100, a1=P(4098)) == ALIGN
    assert f(a7=need - 1) == SHAPE and f(a7=need, a1=P(4098)) == ALIGN
    assert f(a6=P(4096 + 128)) == ALIGN
    all_equal(f, (1, 8), P(4096 + 2), ALIGN)
    all_equal(f, (1, 8), P(4096 + 4), ALIGN, a0=F64)
    assert f(a9=P(4096 + 2)) == ALIGN and f(a10=P(4096 + 4)) == ALIGN                        # int32 counts; int64 inverse
    assert f(a1=None, a0=2) == NULL and f(a0=2, a3=0) == DTYPE and f(a5=101, a1=P(4098)) == SHAPE


def test_voxel_backward(lib):
    # (dtype, grad_centroids, inverse, counts, N, m, M, c, grad_pts, stream)
    f = entry(lib.dicp_voxel_backward, [F32, OK, OK, OK, 2, 100, 40, 3, OK, None])
    all_equal(f, (2, 8, 1, 3), None, NULL)
    assert f(a6=0, a1=None, a3=None, a8=P(4098)) == ALIGN                                    # no voxels: no cotangent / counts asked for
    assert f(a0=2) == DTYPE
    assert f(a4=0) == SHAPE and f(a5=0) == SHAPE and f(a7=2) == SHAPE and f(a6=-1) == SHAPE and f(a6=101) == SHAPE
    assert f(a6=100, a8=P(4098)) == ALIGN
    all_equal(f, (1, 8), P(4096 + 2), ALIGN)
    all_equal(f, (1, 8), P(4096 + 4), ALIGN, a0=F64)
    assert f(a3=P(4096 + 2)) == ALIGN and f(a2=P(4096 + 4)) == ALIGN
    assert f(a2=None, a0=2) == NULL and f(a0=2, a4=0) == DTYPE and f(a6=101, a8=P(4098)) == SHAPE
