"""CPU checks of farthest-point sampling (dicp_amd/fps.py) that need no GPU.

``dicp_amd/csrc/dicp_fps.h`` -- the per-row arithmetic and the comparison rule of the HIP kernels -- is compiled with g++ through
tests/hostcheck/fps_check.cpp, run in a serial loop and held to the numpy restatement tests/fps_ref.py index for index and bit for bit.  The
test clouds are shown to tell the rule from its neighbours (ties the other way, picked rows picked again, the other dtype), the reference's
own invariants are checked, and the argument checks of ``sample_farthest_points`` run before any device work.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dicp_amd import _lib, fps
from dicp_amd.fps import sample_farthest_points

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fps_clouds as fc  # noqa: E402
from fps_ref import fps_ref  # noqa: E402
import hostbuild  # noqa: E402



@pytest.fixture(scope="module")
def check():
    lib = hostbuild.build("fps_check.cpp", "fps_check", ("-Wall",))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    for fn in (lib.fc_run_f32, lib.fc_run_f64):
        fn.argtypes = [vp, i32, i32, ctypes.c_longlong, i32, i32, vp, vp]
        fn.restype = i32
    return lib


def _header(lib, p, k, rows, start, use_key):
    p = np.ascontiguousarray(p)
    idx = np.zeros(k, dtype=np.int64)
    dist = np.zeros(k, dtype=p.dtype)
    fn = lib.fc_run_f32 if p.dtype == np.float32 else lib.fc_run_f64
    keff = fn(p.ctypes.data_as(ctypes.c_void_p), p.shape[1], p.shape[0] if rows is None else rows, start, k, use_key,
              idx.ctypes.data_as(ctypes.c_void_p), dist.ctypes.data_as(ctypes.c_void_p))
    return idx, dist, keff


def _same(a, b):
    """bit for bit (NaN-free arrays of one dtype; +inf equal to +inf)"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _hold(lib, p, k, rows=None, start=0):
    ri, rd, rk = fps_ref(p, k, rows=rows, start=start)
    for use_key in (0, 1):
        hi, hd, hk = _header(lib, p, k, rows, start, use_key)
        assert hk == rk
        assert np.array_equal(hi, ri), np.flatnonzero(hi != ri)[:5]
        assert _same(hd, rd)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_header_matches_reference(check, dtype):
    """fails without dicp_fps.h"""
    for seed, n, k, start in ((10, 1, 3, 0), (11, 2, 2, 1), (12, 777, 300, 5), (13, 5000, 512, 4999), (14, 300, 300, 1234)):
        _hold(check, fc.random_cloud(n, 3, dtype, seed), k, start=start)
    _hold(check, fc.random_cloud(900, 6, dtype, 15), 64, rows=650, start=700)            # extra columns, ragged rows, a start past them
    for n in (300, 5000):
        _hold(check, fc.lattice_cloud(n, dtype), n)
    _hold(check, fc.repeated_point(200, dtype), 200, start=7)
    _hold(check, fc.grid_cloud(9, dtype), 729)
    bad = fc.nonfinite_cloud(700, dtype)
    for start in (0, 5, 699):                                                            # (rows 5 and 699 are non-finite)
        _hold(check, bad, 700, start=start)
    _hold(check, np.full((40, 3), np.nan, dtype=dtype), 5)                               # no candidate at all
    _hold(check, fc.random_cloud(10, 3, dtype, 16), 4, rows=0)
    _hold(check, fc.sphere_cloud().astype(dtype), 400)


def test_header_matches_reference_on_overflow(check):
    p = fc.overflow_cloud()
    d = fps_ref(p, 500)[1]
    assert np.isinf(d[1:]).sum() > 10 and np.isfinite(d).sum() > 10       # +inf is an ordinary value on this cloud, and not the only one
    _hold(check, p, 500)
    _hold(check, p, 64, start=77)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_clouds_tell_the_rule_from_its_neighbours(dtype):
    for p in (fc.lattice_cloud(300, dtype), fc.lattice_cloud(5000, dtype), np.repeat(fc.random_cloud(60, 3, dtype, 20), 4, axis=0)):
        n = p.shape[0]
        true = fps_ref(p, n)[0]
        assert not np.array_equal(fps_ref(p, n, tie_high=True)[0], true)
        assert not np.array_equal(fps_ref(p, n, repick=True)[0], true)


def test_dtypes_differ_on_the_near_tie_cloud():
    p = fc.sphere_cloud()
    i32, i64 = fps_ref(p, 400)[0], fps_ref(p.astype(np.float64), 400)[0]
    assert (i32 != i64).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_invariants(dtype):
    clouds = [fc.random_cloud(1500, 3, dtype, 30), fc.lattice_cloud(300, dtype), fc.repeated_point(200, dtype), fc.grid_cloud(9, dtype),
              fc.nonfinite_cloud(700, dtype), fc.sphere_cloud().astype(dtype)] + ([fc.overflow_cloud()] if dtype == np.float32 else [])
    for p in clouds:
        n = p.shape[0]
        cand = np.flatnonzero(np.isfinite(p[:, :3]).all(1))
        for k in (64, n + 3):
            idx, dist, keff = fps_ref(p, k, start=11)
            assert keff == min(k, cand.size)
            assert (idx[keff:] == -1).all() and np.isinf(dist[keff:]).all() and dist[0] == np.inf
            assert np.unique(idx[:keff]).size == keff                                   # distinct
            assert (dist[2:keff] <= dist[1:keff - 1]).all()                                  # never increasing from pick 1 on
            if k >= cand.size:
                assert np.array_equal(np.sort(idx[:keff]), cand)                        # a permutation of the candidates


def test_module_constants_are_the_librarys():
    _lib.build()
    lib = _lib.load()
    for dtype, dt in ((torch.float32, _lib.F32), (torch.float64, _lib.F64)):
        t, nr, sr = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        lib.dicp_fps_geometry(dt, ctypes.byref(t), ctypes.byref(nr), ctypes.byref(sr))
        assert (t.value, nr.value, sr.value) == (fps.T, fps.NR[dtype], fps.STREAM_ROWS)
        assert lib.dicp_fps_workspace_bytes(dt, 4, nr.value, 8, _lib.FPS_AUTO) == 0                 # resident: no workspace
        assert lib.dicp_fps_workspace_bytes(dt, 4, nr.value + 1, 8, _lib.FPS_AUTO) >= 4 * (nr.value + 1) * 4 * (4 << dt)
        assert lib.dicp_fps_workspace_bytes(dt, 4, 100, 8, _lib.FPS_STREAMED) > 0
    assert fps.NR[torch.float32] >= 16384


def test_entry_points_reject_bad_arguments():
    """null pointers, a bad dtype, k < 1 / n < 1 / c < 3: refused before any launch (no GPU touched)"""
    _lib.build()
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    # dicp_fps_forward(dtype, pts, c, rows, start, N, n, k, form, out, idx, dist, k_eff, workspace, bytes, stream)
    good = [0, one, 3, None, None, 1, 10, 4, 0, one, one, one, one, None, 0, None]

    def fwd(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.dicp_fps_forward(*a)
    assert fwd(a1=None) == 1 and fwd(a9=None) == 1 and fwd(a10=None) == 1 and fwd(a11=None) == 1 and fwd(a12=None) == 1
    assert fwd(a0=7) == 3
    assert fwd(a7=0) == 2 and fwd(a6=0) == 2 and fwd(a2=2) == 2 and fwd(a5=0) == 2
    assert fwd(a8=3) == 4
    assert fwd(a8=_lib.FPS_RESIDENT, a6=fps.NR[torch.float32] + 1) == 2
    assert fwd(a8=_lib.FPS_STREAMED) == 1                                                   # the streamed form needs its workspace
    assert fwd(a8=_lib.FPS_STREAMED, a13=one, a14=16) == 2
    assert fwd(a9=ctypes.c_void_p(258)) == 5
    # dicp_fps_backward(dtype, grad_out, idx, N, n, k, c, grad_pts, stream)
    assert lib.dicp_fps_backward(0, None, one, 1, 10, 4, 3, one, None) == 1 and lib.dicp_fps_backward(0, one, one, 1, 10, 4, 3, None, None) == 1
    assert lib.dicp_fps_backward(5, one, one, 1, 10, 4, 3, one, None) == 3 and lib.dicp_fps_backward(0, one, one, 1, 10, 0, 3, one, None) == 2
    assert lib.dicp_fps_backward(0, one, one, 1, 10, 4, 2, one, None) == 2
    assert lib.dicp_fps_workspace_bytes(9, 1, 10, 4, 0) == 0 and lib.dicp_fps_workspace_bytes(0, 1, 0, 4, 2) == 0


# ------------------------------------------------------------------ argument checks (raise before any device work)
def test_bad_points_raise():
    for pts in (np.zeros((10, 3)), "abc", torch.zeros(10, 3, dtype=torch.int64), torch.zeros(10, 3, dtype=torch.float16), torch.zeros(10, 2),
                torch.zeros(2, 10, 2), torch.zeros(10), torch.zeros(2, 3, 10, 3), [], [torch.zeros(2, 5, 3)], [torch.zeros(10, 3), torch.zeros(5, 4)],
                [torch.zeros(10, 3), torch.zeros(5, 3, dtype=torch.float64)], torch.zeros(0, 10, 3)):
        with pytest.raises(ValueError):
            sample_farthest_points(pts, 4)


@pytest.mark.parametrize("k", [0, -1, True, 2.0, "3", None, 2 ** 31])
def test_bad_k_raises(k):
    with pytest.raises(ValueError):
        sample_farthest_points(torch.zeros(10, 3), k)


def test_bad_rows_raise():
    with pytest.raises(ValueError):
        sample_farthest_points([torch.zeros(10, 3)], 4, rows=[10])
    with pytest.raises(ValueError):
        sample_farthest_points(torch.zeros(10, 3), 4, rows=[10])
    for rows in ([3], [3, 11], [-1, 3], [1.0, 2.0], torch.tensor([True, False]), torch.zeros(2, 1, dtype=torch.int64)):
        with pytest.raises(ValueError):
            sample_farthest_points(torch.zeros(2, 10, 3), 4, rows=rows)


@pytest.mark.parametrize("start", [-1, True, 1.5, None, "first", "Random", torch.tensor([-1, 0]), torch.tensor([0, 1, 2]), torch.tensor([0.0, 1.0]),
                                   torch.tensor(1), torch.tensor([True, False]), [0, 1]])
def test_bad_start_raises(start):
    with pytest.raises(ValueError):
        sample_farthest_points(torch.zeros(2, 10, 3), 4, start=start)


def test_bad_form_raises():
    with pytest.raises(ValueError):
        sample_farthest_points(torch.zeros(10, 3), 4, _form="fast")
    with pytest.raises(ValueError):
        sample_farthest_points(torch.zeros(fps.NR[torch.float64] + 1, 3, dtype=torch.float64), 4, _form="resident")
