"""Shared by tests/test_gridknn_host.py (CPU) and tests/test_gpu_knn_grid.py (GPU): the host build of dicp_amd/csrc/dicp_gridknn.h
(tests/hostcheck/gridknn_check.cpp), the clouds of the grid k-NN tests and the comparison with the brute force walk_layouts.knn_oracle.

A plain module (no fixtures): the tests put this directory on sys.path and import it.
"""
import ctypes
import functools

import numpy as np

import ball_clouds as bc
import hostbuild
from walk_layouts import knn_oracle

KS = bc.KS
STATS = ("enlarged", "flat", "visited", "live", "max_passes", "grew", "closed", "whole", "passes", "bound")


@functools.lru_cache(maxsize=None)
def library():
    lib = hostbuild.build("gridknn_check.cpp", "gridknn_check", ("-Wall",))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    for fn, real in ((lib.gk_run_f32, ctypes.c_float), (lib.gk_run_f64, ctypes.c_double)):
        fn.argtypes = [vp, i32, i32, i32, vp, i32, i32, i32, i32, real, vp, vp, vp]
        fn.restype = None
    return lib


def header(x, y, k, x_rows=None, y_rows=None, edge=0.0):
    """The header's scan of every query of x over the host-built grid of y -> ((d2 (n,k), idx (n,k)), stats by name).
    edge: the starting cell edge; 0 for the density rule, as the kernels"""
    lib = library()
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    n, m = x.shape[0], y.shape[0]
    d2 = np.zeros((n, k), dtype=x.dtype)
    idx = np.zeros((n, k), dtype=np.int64)
    stats = np.zeros(len(STATS), dtype=np.int64)
    fn = lib.gk_run_f32 if x.dtype == np.float32 else lib.gk_run_f64
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fn(p(x), n, x.shape[1], n if x_rows is None else x_rows, p(y), m, y.shape[1], m if y_rows is None else y_rows, k, float(x.dtype.type(edge)), p(d2), p(idx), p(stats))
    return (d2, idx), dict(zip(STATS, stats.tolist()))


def reference(x, y, k, x_rows=None, y_rows=None):
    """knn_oracle on columns 0:3 of the rows that take part; +inf / -1 for the query rows at or past x_rows"""
    n = x.shape[0]
    nb = n if x_rows is None else x_rows
    d2 = np.full((n, k), np.inf, dtype=x.dtype)
    idx = np.full((n, k), -1, dtype=np.int64)
    yy = np.ascontiguousarray(y[:y.shape[0] if y_rows is None else y_rows, :3])
    if nb:
        d2[:nb], idx[:nb] = knn_oracle(np.ascontiguousarray(x[:nb, :3]), yy, k)
    return d2, idx


def same(got, ref):
    """None when idx agrees index for index and d2 bit for bit, else a description of the first difference"""
    (d2, idx), (rd2, ridx) = got, ref
    if d2.shape != rd2.shape or idx.shape != ridx.shape or d2.dtype != rd2.dtype:
        return "shapes / dtypes differ"
    bad = np.flatnonzero((idx != ridx).any(1))
    if bad.size:
        return "%d queries differ in idx, first %d: %s against %s" % (bad.size, bad[0], idx[bad[0]], ridx[bad[0]])
    if d2.tobytes() != rd2.tobytes():
        bad = np.flatnonzero((d2.view(np.uint8).reshape(d2.shape[0], -1) != rd2.view(np.uint8).reshape(d2.shape[0], -1)).any(1))
        return "%d queries differ in the bits of d2, first %d: %s against %s" % (bad.size, bad[0], d2[bad[0]], rd2[bad[0]])
    return None


def further_cases(dtype):
    """(name, x, y): k above the live-row count, a cluster smaller than k facing a far cluster, queries 1e6 extents away, float32
    queries whose d2 overflows"""
    rng = np.random.default_rng(12)
    out = []
    x, y = bc.random_pair(50, 5, dtype, seed=9)
    y[3] = np.nan
    out.append(("k above the live rows", x, y))
    near = rng.random((5, 3)) * 0.01
    far = rng.random((400, 3)) * 0.5 + 40.0
    q = np.concatenate([rng.random((40, 3)) * 0.01, rng.random((10, 3)) * 0.5 + 40.0])
    out.append(("small cluster facing a far one", q.astype(dtype), np.concatenate([near, far]).astype(dtype)))
    _, y = bc.random_pair(1, 600, dtype, seed=10)
    q = rng.random((30, 3)) + np.repeat(np.array([[1e6, 0, 0], [0, -1e6, 0], [1e6, 1e6, 1e6]]), 10, 0)
    out.append(("queries 1e6 extents away", np.concatenate([q, rng.random((5, 3))]).astype(dtype), y))
    if dtype == np.float32:
        q = np.array([[1e30, 0.5, 0.5], [0.5, -1e30, 0.5], [1e30, 1e30, 1e30], [3e38, -3e38, 3e38], [0.5, 0.5, 0.5]], dtype)
        out.append(("queries at 1e30", q, y))
    return out


def all_cases(dtype):
    """(name, x, y) of every layout but the random cubes: the lattice, the degenerate layouts, the further cases and the flat plan"""
    out = [(name, x, y) for name, x, y, r in bc.lattice_cases(dtype) if "r=" not in name or name.endswith("r=1.0") or name.endswith("r=1")]
    out += [(name, x, y) for name, x, y, _ in bc.degenerate_cases(dtype)]
    out += further_cases(dtype)
    big = np.array([[3.0e38, 0, 0], [-3.0e38, 0, 0], [0, 0, 0], [0, 1, 0]], dtype=dtype)
    out.append(("extent 3e38", big[2:], big))
    return out
