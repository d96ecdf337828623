"""CPU checks of the voxel-grid downsample (dicp_amd/voxel.py) that need no GPU.

``dicp_amd/csrc/dicp_voxel.h`` -- the per-point key arithmetic of the HIP kernels -- is compiled with g++ through
tests/hostcheck/voxel_check.cpp and held to numpy: coordinates floor((p - o) / s) in the points' dtype, bit widths, keys and the
64-bit limit.  The argument checks of ``voxel_downsample`` run before any device work.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd.voxel import voxel_downsample

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostbuild  # noqa: E402


@pytest.fixture(scope="module")
def vc():
    lib = hostbuild.build("voxel_check.cpp", "voxel_check")
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    lib.vc_coord_f32.argtypes = [vp, i32, ctypes.c_float, ctypes.c_float, vp, vp]
    lib.vc_coord_f64.argtypes = [vp, i32, ctypes.c_double, ctypes.c_double, vp, vp]
    lib.vc_coord_f32.restype = lib.vc_coord_f64.restype = None
    lib.vc_width.argtypes = [i64, i64]
    lib.vc_width.restype = i32
    lib.vc_widths_ok.argtypes = lib.vc_passes.argtypes = [i32, i32, i32]
    lib.vc_widths_ok.restype = lib.vc_passes.restype = i32
    lib.vc_keys.argtypes = [vp, i32, vp, i32, i32, vp]
    lib.vc_keys.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _coords(vc, p, o, s):
    """the header's coordinates of the 1-D array p (its own dtype) -> (v int64, ok bool)"""
    p = np.ascontiguousarray(p)
    v = np.zeros(p.shape[0], dtype=np.int64)
    ok = np.zeros(p.shape[0], dtype=np.int32)
    fn = vc.vc_coord_f32 if p.dtype == np.float32 else vc.vc_coord_f64
    fn(_p(p), p.shape[0], float(p.dtype.type(o)), float(p.dtype.type(s)), _p(v), _p(ok))
    return v, ok.astype(bool)


def _oracle_coords(p, o, s):
    dt = p.dtype.type
    return np.floor((p - dt(o)) / dt(s))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_coordinates_match_numpy(vc, dtype):
    rng = np.random.default_rng(1)
    for o, s, scale in ((0.0, 0.1, 50.0), (-3.7, 0.05, 20.0), (2500.0, 0.07, 2600.0), (1.25, 0.3, 1e4)):
        p = (rng.standard_normal(20000) * scale).astype(dtype)
        v, ok = _coords(vc, p, o, s)
        ref = _oracle_coords(p, o, s)
        assert ok.all()
        assert np.array_equal(v, ref.astype(np.int64))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_negative_coordinates_floor(vc, dtype):
    p = np.array([-0.01, -0.25, -0.2500001, -1.0, -1e-30, 0.0, -0.0, 0.24], dtype=dtype)
    v, ok = _coords(vc, p, 0.0, 0.25)
    assert ok.all()
    assert np.array_equal(v, _oracle_coords(p, 0.0, 0.25).astype(np.int64))
    assert v[0] == -1 and v[1] == -1 and v[3] == -4 and v[4] == -1 and v[5] == 0 and v[6] == 0 and v[7] == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_points_on_voxel_faces(vc, dtype):
    k = np.arange(-400, 401)
    p = (k * 0.25).astype(dtype)                            # every point exactly on a face (representable with s = 0.25)
    v, ok = _coords(vc, p, 0.0, 0.25)
    assert ok.all() and np.array_equal(v, k)
    v, ok = _coords(vc, p + dtype(0.5), 0.5, 0.25)          # and with an origin on a face too
    assert np.array_equal(v, k)


def test_coordinate_limit(vc):
    lim = 2.0 ** 62
    p = np.array([lim - 2 ** 10, lim, -lim, -lim + 2 ** 10, np.inf, -np.inf, 1e300], dtype=np.float64)
    v, ok = _coords(vc, p, 0.0, 1.0)
    assert list(ok) == [True, False, False, True, False, False, False]
    assert v[0] == int(lim) - 2 ** 10 and v[3] == -int(lim) + 2 ** 10
    p32 = np.array([1e30, 1.0], dtype=np.float32)
    _, ok = _coords(vc, p32, 0.0, np.float32(1e-10))
    assert list(ok) == [False, True]


def test_widths(vc):
    rng = np.random.default_rng(2)
    cases = [(0, 0), (-5, -5), (0, 1), (-1, 0), (-(2 ** 62) + 1, 2 ** 62 - 1), (3, 2 ** 40)]
    cases += [tuple(sorted(int(x) for x in rng.integers(-(2 ** 61), 2 ** 61, 2))) for _ in range(200)]
    for lo, hi in cases:
        assert vc.vc_width(lo, hi) == (hi - lo).bit_length(), (lo, hi)


def test_64_bit_limit_at_its_edge(vc):
    assert vc.vc_widths_ok(22, 21, 21) == 1 and vc.vc_widths_ok(64, 0, 0) == 1 and vc.vc_widths_ok(0, 0, 64) == 1
    assert vc.vc_widths_ok(22, 21, 22) == 0 and vc.vc_widths_ok(63, 1, 1) == 0
    assert [vc.vc_passes(*w) for w in ((0, 0, 0), (1, 0, 0), (3, 3, 2), (3, 3, 3), (22, 21, 21))] == [0, 1, 1, 2, 8]


def _keys(vc, v, lo, wy, wz):
    v = np.ascontiguousarray(v, dtype=np.int64)
    lo = np.ascontiguousarray(lo, dtype=np.int64)
    key = np.zeros(v.shape[0], dtype=np.uint64)
    vc.vc_keys(_p(v), v.shape[0], _p(lo), wy, wz, _p(key))
    return key


@pytest.mark.parametrize("spans", [(5, 7, 3), (1, 1, 1), (0, 9, 0), (2 ** 21, 2 ** 20, 2 ** 20), (2 ** 63 - 2, 0, 0), (0, 0, 2 ** 63 - 2)])
def test_keys_sort_lexicographically(vc, spans):
    rng = np.random.default_rng(sum(spans) % 1000)
    lo = np.array([-(s // 2) for s in spans], dtype=np.int64)
    v = np.stack([lo[d] + rng.integers(0, spans[d] + 1, 3000, dtype=np.int64) for d in range(3)], 1)
    v[0] = lo
    v[1] = lo + np.array(spans, dtype=np.int64)             # both ends of every axis: the widths are exact
    w = [int(s).bit_length() for s in spans]
    assert sum(w) <= 64
    key = _keys(vc, v, lo, w[1], w[2])
    order = np.argsort(key, kind="stable")
    uniq, inv = np.unique(v, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    assert np.array_equal(v[order], v[np.lexsort((np.arange(v.shape[0]), v[:, 2], v[:, 1], v[:, 0]))])
    # equal keys exactly for equal coordinates
    ukey = _keys(vc, uniq, lo, w[1], w[2])
    assert np.array_equal(key, ukey[inv]) and np.unique(ukey).shape[0] == uniq.shape[0]


# ------------------------------------------------------------------ argument checks (raise before any device work)
@pytest.mark.parametrize("size", [0.0, -0.1, float("nan"), float("inf"), [0.1, 0.0, 0.1], [0.1, 0.1], torch.zeros(2, 3) + 0.1, True, "a", 1e-50])
def test_bad_voxel_size_raises(size):
    with pytest.raises(ValueError):
        voxel_downsample(torch.zeros(10, 3), size)


def test_voxel_size_overflowing_float32_raises():
    with pytest.raises(ValueError):
        voxel_downsample(torch.zeros(10, 3), 1e300)
    with pytest.raises(ValueError):
        voxel_downsample(torch.zeros(10, 3), [0.1, 0.1, 1e-60])


@pytest.mark.parametrize("origin", [torch.zeros(2), torch.zeros(3, 3), [0.0, float("nan"), 0.0], [float("inf")] * 3, 1.0, [1e300, 0.0, 0.0], "abc"])
def test_bad_origin_raises(origin):
    with pytest.raises(ValueError):
        voxel_downsample(torch.zeros(2, 10, 3), 0.1, origin=origin)


@pytest.mark.parametrize("mp", [0, -1, 1.5, True, "2", None])
def test_bad_min_points_raises(mp):
    with pytest.raises(ValueError):
        voxel_downsample(torch.zeros(10, 3), 0.1, min_points=mp)


def test_bad_points_raise():
    for pts in (torch.zeros(10, 2), torch.zeros(10, 3, dtype=torch.int64), torch.zeros(10, 3, dtype=torch.float16), torch.zeros(2, 10, 3, 1),
                torch.zeros(10), torch.zeros(0, 3), torch.zeros(2, 0, 3), np.zeros((10, 3)), [], [torch.zeros(0, 3)],
                [torch.zeros(10, 3), torch.zeros(5, 4)], [torch.zeros(10, 3), torch.zeros(5, 3, dtype=torch.float64)], [torch.zeros(2, 5, 3)]):
        with pytest.raises(ValueError):
            voxel_downsample(pts, 0.1)


def test_bad_rows_raise():
    for rows in ([3], [3, 11], [-1, 3], [1.0, 2.0], torch.tensor([True, False])):
        with pytest.raises(ValueError):
            voxel_downsample(torch.zeros(2, 10, 3), 0.1, rows=rows)
    with pytest.raises(ValueError):
        voxel_downsample([torch.zeros(10, 3)], 0.1, rows=[10])
