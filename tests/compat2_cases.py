"""What the CPU and the GPU tests of second_order_compatibility / consensus_correspondences share: the ctypes front of the g++ build of
csrc/dicp_compat2.h and the designed inputs.

A plain module (no fixtures): the tests put this directory on sys.path and import it.
"""
import ctypes

import numpy as np

import compat2_ref as c2
import hostbuild
import ransac_ref as rr

P_, I, F64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
SFX = {np.float32: "f32", np.float64: "f64"}


def build():
    lib = hostbuild.build("compat2_check.cpp", "compat2_check", ("-Wall",))
    lib.c2_words.restype, lib.c2_words.argtypes = I, [I]
    lib.c2_second.restype, lib.c2_second.argtypes = None, [P_, I, I, P_, P_]
    lib.c2_rank.restype, lib.c2_rank.argtypes = None, [P_, I, P_]
    lib.c2_members.restype, lib.c2_members.argtypes = None, [P_, I, I, P_, I, I, P_]
    for s in SFX.values():
        getattr(lib, "c2_bits_" + s).restype = None
        getattr(lib, "c2_bits_" + s).argtypes = [P_, I, I, F64, F64, P_, P_]
        getattr(lib, "c2_score_" + s).restype = None
        getattr(lib, "c2_score_" + s).argtypes = [P_, I, P_]
        getattr(lib, "c2_fit_" + s).restype = None
        getattr(lib, "c2_fit_" + s).argtypes = [P_, P_, I, I, P_, P_]
    return lib


def _ptr(a):
    return a.ctypes.data_as(P_)


def header_stages(lib, pairs, n, threshold, min_length, seeds, members):
    """the header's lines on one cloud's packed pairs (P, 6) -> dict adj (n, W) int64, degree (n,) int32, S (P, P) int32, degree2 (P,)
    int64, rank2 (P,) int32, score2 (P,) T, lists (seeds, members) int32, sums (seeds, 18) float64, poses (seeds, 12) T"""
    pairs = np.ascontiguousarray(pairs)
    dt = pairs.dtype
    s = SFX[dt.type]
    P, W = pairs.shape[0], c2.words(n)
    adj, degree = np.empty((n, W), np.int64), np.empty(n, np.int32)
    getattr(lib, "c2_bits_" + s)(_ptr(pairs), P, n, float(threshold), float(min_length), _ptr(adj), _ptr(degree))
    S, d2 = np.empty((P, P), np.int32), np.empty(P, np.int64)
    lib.c2_second(_ptr(adj), P, n, _ptr(S), _ptr(d2))
    rank2, score2 = np.empty(P, np.int32), np.empty(P, dt)
    lib.c2_rank(_ptr(d2), P, _ptr(rank2))
    getattr(lib, "c2_score_" + s)(_ptr(d2), P, _ptr(score2))
    lists = np.empty((seeds, members), np.int32)
    lib.c2_members(_ptr(adj), P, n, _ptr(rank2), seeds, members, _ptr(lists))
    sums, poses = np.empty((seeds, 18), np.float64), np.empty((seeds, 12), dt)
    getattr(lib, "c2_fit_" + s)(_ptr(pairs), _ptr(lists), seeds, members, _ptr(sums), _ptr(poses))
    return dict(adj=adj, degree=degree, S=S, degree2=d2, rank2=rank2, score2=score2, lists=lists, sums=sums, poses=poses)


def header_fit(lib, pairs, lists):
    """-> sums (H, 18), poses (H, 12) T of given member lists (H, K) int32"""
    pairs, lists = np.ascontiguousarray(pairs), np.ascontiguousarray(lists, dtype=np.int32)
    sums, poses = np.empty((lists.shape[0], 18), np.float64), np.empty((lists.shape[0], 12), pairs.dtype)
    getattr(lib, "c2_fit_" + SFX[pairs.dtype.type])(_ptr(pairs), _ptr(lists), lists.shape[0], lists.shape[1], _ptr(sums), _ptr(poses))
    return sums, poses


def motion_cloud(rng, n, m, P, dtype, inliers, noise=0.004, rows=None):
    """One cloud with exactly P live pairs among its first `rows` rows, `inliers` of them (at most) under one rigid motion in a 4-unit
    cube and the rest matched at random; the other rows are not live (idx < 0, a NaN in x, an inf in the matched y in turn); the rows at
    and past `rows` are padding holding NaN and 1e30 with idx in or out of range.  -> x (n, 3), y (m, 3), idx (n,) int64"""
    rows = n if rows is None else rows
    C, r = rr.rotation(rng), rng.uniform(-0.5, 0.5, 3)
    x = rng.uniform(0.0, 4.0, (n, 3))
    to = rng.permutation(m)[:n] if n <= m else rng.integers(0, m, n)
    y = rng.uniform(0.0, 4.0, (m, 3))
    livepos = np.sort(rng.permutation(rows)[:P])
    good = livepos[rng.permutation(P)[:min(inliers, P)]]
    y[to[good]] = x[good] @ C.T + r + noise * rng.standard_normal((good.size, 3))
    idx = to.astype(np.int64)
    x, y = x.astype(dtype), y.astype(dtype)
    dead = np.setdiff1d(np.arange(rows), livepos)
    for k, i in enumerate(dead):
        if k % 3 == 0:
            idx[i] = -1 - (k % 5)
        elif k % 3 == 1:
            x[i, k % 3] = np.nan
        elif n <= m and not np.isin(to[i], to[livepos]):
            y[idx[i], 2] = np.inf
        else:
            idx[i] = -1
    x[rows:] = np.nan
    x[rows + 1::2] = 1e30
    idx[rows:] = rng.integers(-3, m + 40, n - rows)
    return x, y, idx
