"""Shared by tests/test_normals_grid_host.py (CPU) and tests/test_gpu_normals_grid.py (GPU): the host build of the density plan and the
cell keys of a cloud (tests/hostcheck/gridorder_check.cpp, the header the grid build runs), the order of the grid from them, a numpy model
of estimate_normals' backward window in that order, and the clouds of the method="grid" tests.

The window model is only used to PROVE that a test input reaches the code it is meant for (the share of the backward's entries that
leave the LDS window); it is never the expected value of anything.

A plain module (no fixtures): the tests put this directory on sys.path and import it.
"""
import ctypes
import functools

import numpy as np

import hostbuild
import walk_layouts as wl

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


@functools.lru_cache(maxsize=None)
def library():
    lib = hostbuild.build("gridorder_check.cpp", "gridorder_check", ("-Wall",))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    for fn in (lib.go_keys_f32, lib.go_keys_f64):
        fn.argtypes = [vp, i32, i32, i32, vp, vp, vp]
        fn.restype = None
    return lib


class GridOrder:
    """keys (m,) uint64 in the original row order (NO_KEY: the row stays out of the grid); cnt live rows; flat; perm (m,): the row of
    every sorted slot, the pairs sorted by (key, original index) as the device sort does -- slots 0 .. cnt - 1 the live rows, the others
    after them in index order; slot (m,) its inverse"""


def grid_order(P, rows=None):
    P = np.ascontiguousarray(P)
    assert P.dtype in (np.float32, np.float64) and P.ndim == 2 and P.shape[1] >= 3
    m = P.shape[0]
    g = GridOrder()
    g.keys = np.zeros(m, dtype=np.uint64)
    plan = np.zeros(7, dtype=np.int64)
    edge = np.zeros(4, dtype=np.float64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fn = library().go_keys_f32 if P.dtype == np.float32 else library().go_keys_f64
    fn(p(P), m, P.shape[1], m if rows is None else int(rows), p(g.keys), p(plan), p(edge))
    g.cnt, g.flat, g.hi, g.edge = int(plan[0]), int(plan[1]), plan[2:5].tolist(), float(edge[0])
    g.perm = np.lexsort((np.arange(m), g.keys))
    g.slot = np.empty(m, dtype=np.int64)
    g.slot[g.perm] = np.arange(m)
    assert int((g.keys != NO_KEY).sum()) == g.cnt
    return g


def grid_windows(P, k, dtype, nbr, rows=None):
    """The backward window of csrc/normals.hip in the grid's order: the block of BLOCK slots of a query and H slots on either side,
    cut at the live rows.  P in the dtype under test, nbr (m,k) neighbour lists (-1: empty) -> wl.NormalsWindows"""
    dt = wl.np_dtype(dtype)
    H = wl.HALO[dt]
    g = grid_order(np.asarray(P).astype(dt), rows)
    m = P.shape[0]
    nbr = np.asarray(nbr)
    kept = nbr >= 0
    j = np.where(kept, g.slot[np.clip(nbr, 0, m - 1)], -1)
    s0 = (g.slot // wl.BLOCK) * wl.BLOCK
    wlo = np.maximum(s0 - H, 0)[:, None]
    whi = np.minimum(s0 + wl.BLOCK + H, g.cnt)[:, None]
    w = wl.NormalsWindows()
    w.kept = kept
    w.bwd_outside = kept & ((j < wlo) | (j >= whi))
    w.indegree = np.bincount(nbr[kept], minlength=m)
    return w


# ---------------------------------------------------------------- the layouts of the gradient tests
# (name, dtype name) -> (points float64, k).  In grid order a planar layout stays inside the window up to 40000 rows (a wall is one cell
# in x: its slots run along y, and a neighbourhood spans a few columns of cells), so the out-of-window cases are the two cubes.
GRAD_LAYOUTS = (("cube", "float32"), ("cube", "float64"), ("wall", "float32"), ("wall", "float64"))
K_GRAD = 16


def grad_layout(name, dtype):
    dt = wl.np_dtype(dtype)
    if name == "cube":
        return wl.cube(40000 if dt == np.float32 else 20000, 0).astype(dt)
    if name == "wall":
        return wl.wall(6000, 0).astype(dt)
    raise KeyError(name)


def check_grad_conditions(name, w):
    """The conditions a layout has to meet before a test may look at a GPU result"""
    s = w.share()
    if name == "cube":
        assert s >= 0.2 and 1.0 - s >= 0.2, (name, s)
    elif name == "wall":
        assert not w.bwd_outside.any(), (name, s)
    else:
        raise KeyError(name)
    return s
