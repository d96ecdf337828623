"""What the CPU and the GPU tests of ransac_correspondences share: the ctypes front of the g++ build of csrc/dicp_ransac.h, the comparison
of stored poses with the float64 numpy Kabsch, and its bound.

THE BOUND OF A STORED POSE.  A pose value v is rounded once to T: u_T |v|.  Before that it is double arithmetic on raw (un-centred)
moments: with s the largest |coordinate| of the three pairs, the covariance W = M / 3 - mu_t mu_s^T carries an absolute error of a few
2^-53 s^2, and the rotation of a rank-2 W moves by dW over W's second singular value w_2 (small when the source OR the target triple is
nearly collinear): dC <= K_C g with g = 2^-53 s^2 / w_2, and dr <= K_R g s (r = mu_t - C mu_s).  K_C and K_R are 16
times the largest normalised errors of the host build against the numpy reference (profiles/r26_ransac_edges.txt, written by
scripts/ransac_edges.py: uniform cubes at the origin and 2.5 km away, both dtypes, 20 000 triples each); the factor covers the fma
contraction of the device build.  Only triples whose centred source triple has sigma_2 / sigma_1 >= 0.1 are compared (a near-collinear triple has no stable
rotation), and the callers assert that at least 90 % qualify.

A plain module (no fixtures): the tests put this directory on sys.path and import it.
"""
import ctypes

import numpy as np

import hostbuild
import ransac_ref as rr

P_, I, U32, F64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_double
SFX = {np.float32: "f32", np.float64: "f64"}
U_T = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
K_C, K_R = 16 * 3.51, 16 * 4.02       # 16 x the largest normalised errors of profiles/r26_ransac_edges.txt
MIN_RATIO, MIN_SHARE = 0.1, 0.9


def build():
    lib = hostbuild.build("ransac_check.cpp", "ransac_check", ("-Wall",))
    lib.rc_mix32.restype, lib.rc_mix32.argtypes = U32, [U32]
    lib.rc_draws.restype, lib.rc_draws.argtypes = None, [U32, U32, U32, P_]
    lib.rc_positions.restype, lib.rc_positions.argtypes = None, [U32, U32, U32, U32, P_]
    lib.rc_fma.restype, lib.rc_fma.argtypes = F64, [F64] * 3
    for s in SFX.values():
        getattr(lib, "rc_hypotheses_" + s).restype = None
        getattr(lib, "rc_hypotheses_" + s).argtypes = [P_, I, I, U32, U32, P_, P_, P_]
        getattr(lib, "rc_score_" + s).restype = None
        getattr(lib, "rc_score_" + s).argtypes = [P_, I, P_, I, F64, P_, P_, P_, P_]
        getattr(lib, "rc_live_" + s).restype = I
        getattr(lib, "rc_live_" + s).argtypes = [I, ctypes.c_int64, P_, P_]
    return lib


def _ptr(a):
    return a.ctypes.data_as(P_)


def header_hypotheses(lib, pairs, H, seed, cloud=0):
    """-> samples (H, 3) int32, sums (H, 18) float64, poses (H, 12) T of one cloud's packed pairs (P >= 3)"""
    pairs = np.ascontiguousarray(pairs)
    smp, sm, ps = np.empty((H, 3), np.int32), np.empty((H, 18), np.float64), np.empty((H, 12), pairs.dtype)
    getattr(lib, "rc_hypotheses_" + SFX[pairs.dtype.type])(_ptr(pairs), pairs.shape[0], H, seed & 0xFFFFFFFF, cloud, _ptr(smp), _ptr(sm), _ptr(ps))
    return smp, sm, ps


def header_score(lib, pairs, poses, threshold):
    """-> d (H, P) T, counts (H,) int32, best, best_count"""
    pairs, poses = np.ascontiguousarray(pairs), np.ascontiguousarray(poses, dtype=pairs.dtype)
    H, P = poses.shape[0], pairs.shape[0]
    d, counts = np.empty((H, P), pairs.dtype), np.empty(H, np.int32)
    best, bc = np.empty(1, np.int32), np.empty(1, np.int32)
    getattr(lib, "rc_score_" + SFX[pairs.dtype.type])(_ptr(pairs), P, _ptr(poses), H, float(threshold), _ptr(d), _ptr(counts), _ptr(best), _ptr(bc))
    return d, counts, int(best[0]), int(bc[0])


def same_bits(a, b):
    """equal bit for bit (signed zeros told apart), NaN in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a).astype(a.dtype).view(u), np.where(nb, 0, b).astype(a.dtype).view(u)))


def cube_pairs(rng, P, dtype, offset=0.0, noise=0.0):
    """P packed pairs: x uniform in a unit cube at `offset` along every axis, y = C x + r (+ noise), in dtype"""
    C, r = rr.rotation(rng), rng.uniform(-0.5, 0.5, 3)
    x = (rng.uniform(-0.5, 0.5, (P, 3)) + offset).astype(dtype)
    y = (x.astype(np.float64) @ C.T + r + noise * rng.standard_normal((P, 3))).astype(dtype)
    return np.concatenate((x, y), axis=1)


def pose_errors(poses, pairs, abc):
    """stored poses (H, 12) T of the triples abc (H, 3) of packed pairs -> (normalised dC (H,), normalised dr (H,), qualifies (H,) bool):
    the error beyond the one rounding to T, in units of g and g s (see the module's docstring)"""
    dt = pairs.dtype.type
    tri = pairs[abc].astype(np.float64)
    ref, sig, sw = rr.kabsch(tri[:, :, :3], tri[:, :, 3:])
    ok = sig[:, 1] >= MIN_RATIO * sig[:, 0]
    s = np.abs(tri).max(axis=(1, 2))
    with np.errstate(all="ignore"):
        g = 2.0 ** -53 * s * s / sw[:, 1]
        err = np.maximum(np.abs(np.asarray(poses, dtype=np.float64) - ref) - U_T[dt] * np.abs(ref), 0.0)
        return err[:, :9].max(axis=1) / g, err[:, 9:].max(axis=1) / (g * s), ok


def poses_hold(poses, pairs, abc):
    """-> (all qualifying poses inside the bound, the share that qualifies, worst dC / K_C, worst dr / K_R)"""
    eC, eR, ok = pose_errors(poses, pairs, abc)
    if not ok.any():
        return False, 0.0, np.inf, np.inf
    wc, wr = float(eC[ok].max()) / K_C, float(eR[ok].max()) / K_R
    return bool(wc <= 1.0 and wr <= 1.0), float(ok.mean()), wc, wr
