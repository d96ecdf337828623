"""What the CPU and the GPU tests of gnc_correspondences share: the ctypes front of the g++ build of csrc/dicp_gnc.h, the comparison of
a round's pose with the float64 numpy Kabsch of its weights, the designed inputs and the recovery cases with their limits.

THE BOUND OF A ROUND'S POSE is that of tests/ransac_cases.py for the closed form, with the same constants K_C and K_R: the pose stays in
double here (no rounding to T), and with s the largest |coordinate| of the pairs that carry weight and w_2 the second singular value of
their weighted covariance, dC <= K_C g and dr <= K_R g s with g = 2^-53 s^2 / w_2.

THE RECOVERY LIMITS are twice the largest rotation error the g++ build itself shows on each family of runs
(profiles/r32_gnc_edges.txt, written by scripts/gnc_edges.py): five seeds x two inlier counts x two losses per family.

A plain module (no fixtures): the tests put this directory on sys.path and import it.
"""
import ctypes

import numpy as np

import compat_ref as cr
import gnc_ref as gr
import hostbuild
import ransac_cases as rc
import ransac_ref as rr

P_, I, F64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
SFX = rc.SFX
same_bits = rc.same_bits
DTYPES = [np.float32, np.float64]

# twice the largest error of the g++ build on each family (profiles/r32_gnc_edges.txt)
LIMIT_COMPAT = 2 * 4.195e-4           # compat_ref.recovery_case(seed, inliers=300 / 180), threshold 0.05
LIMIT_RANSAC = 2 * 2.460e-3           # ransac_ref.recovery_case(seed) and (seed, inlier_ratio=0.25), threshold 0.02
LEAST_SQUARES_FLOOR = 0.02            # the fit over every match is further than this from the truth on every recovery case


def build():
    lib = hostbuild.build("gnc_check.cpp", "gnc_check", ("-Wall", "-ffp-contract=off"))
    for name in ("gc_slots", "gc_iter_max", "gc_trace"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = I, []
    lib.gc_bad_arguments.restype, lib.gc_bad_arguments.argtypes = I, [I, F64, F64, I]
    lib.gc_weight.restype, lib.gc_weight.argtypes = None, [I, F64, F64, F64, P_]
    for s in SFX.values():
        getattr(lib, "gc_residual_" + s).restype, getattr(lib, "gc_residual_" + s).argtypes = F64, [P_, P_]
        getattr(lib, "gc_fit_" + s).restype, getattr(lib, "gc_fit_" + s).argtypes = I, [P_, I, P_, I, F64, F64, I, P_, P_, P_, P_, P_, P_, P_]
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(P_)


def header_weight(lib, loss, mu, c2, d):
    """-> lo, hi, w, band of one pair"""
    out = np.empty(4)
    lib.gc_weight(loss, float(mu), float(c2), float(d), _ptr(out))
    return float(out[0]), float(out[1]), float(out[2]), int(out[3])


def header_fit(lib, pairs, u, loss, threshold, growth=1.4, iterations=128, detail=False):
    """dicp_gnc_fit's outputs for one cloud's packed pairs from the g++ build -> dict: weights (P,) T, rounds, status, mu,
    pose_last (12,) T, trace (iterations + 1, 32) float64 (zeros past the last record), and with detail d and w (iterations + 1, P)"""
    pairs = np.ascontiguousarray(pairs)
    P, dt = pairs.shape[0], pairs.dtype
    u = None if u is None else np.ascontiguousarray(u, dtype=dt)
    w, pose = np.zeros(P, dt), np.zeros(12, dt)
    rounds, status, mu = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1)
    trace = np.zeros((iterations + 1, gr.TRACE))
    det = np.zeros((iterations + 1, 2, max(P, 1))) if detail else None
    code = getattr(lib, "gc_fit_" + SFX[dt.type])(_ptr(pairs), P, _ptr(u), loss, float(threshold), float(growth), int(iterations), _ptr(w), _ptr(rounds),
                                                  _ptr(status), _ptr(mu), _ptr(pose), _ptr(trace), _ptr(det))
    assert code == 0, code
    out = dict(weights=w, rounds=int(rounds[0]), status=int(status[0]), mu=float(mu[0]), pose_last=pose, trace=trace)
    if detail:
        out.update(d=det[:, 0, :P], w=det[:, 1, :P])
    return out


def header_call(lib, x, y, idx, threshold, loss="tls", growth=1.4, iterations=128, weight=None, x_rows=None):
    """gnc_correspondences' kernel outputs for one cloud from the g++ build, in the original row order -> header_fit's dict with
    weights (n,) T (0 on rows that are not live), and rows, pairs, u"""
    rows, pairs, u = gr.packed(x, y, idx, weight, x_rows)
    out = header_fit(lib, pairs, u, gr.LOSSES[loss], threshold, growth, iterations)
    w = np.zeros(x.shape[0], x.dtype)
    w[rows] = out["weights"]
    return dict(out, weights=w, rows=rows, pairs=pairs, u=u)


def pose_holds(pose, pairs, omega):
    """a round's float64 pose against the numpy Kabsch of the weights it was fitted to -> (inside the bound, dC / K_C, dr / K_R)"""
    ref, _, sw = gr.fit_of(pairs, omega)
    s = np.abs(pairs[omega > 0].astype(np.float64)).max()
    with np.errstate(all="ignore"):
        g = 2.0 ** -53 * s * s / sw[1]
        err = np.abs(np.asarray(pose, dtype=np.float64) - ref)
        wc, wr = float(err[:9].max() / g) / rc.K_C, float(err[9:].max() / (g * s)) / rc.K_R
    return bool(wc <= 1.0 and wr <= 1.0), wc, wr


# ------------------------------------------------------------------ inputs
def noisy_cloud(rng, P, dtype, inlier_ratio=0.6, noise=0.01):
    """P packed pairs: x in a unit cube around (1, 1, 1), y = C x + r + noise for the inliers and uniform for the rest"""
    C, r = rr.rotation(rng), rng.uniform(-0.5, 0.5, 3)
    x = rng.uniform(0.5, 1.5, (P, 3))
    y = rng.uniform(-1.0, 3.0, (P, 3))
    good = rng.random(P) < inlier_ratio
    good[:min(P, 4)] = True
    y[good] = x[good] @ C.T + r + noise * rng.standard_normal((int(good.sum()), 3))
    return np.concatenate((x, y), axis=1).astype(dtype)


def rows_cloud(rng, P, extra, dtype, m_extra=30):
    """A cloud with exactly P live rows among n = P + extra: the dead rows are interleaved, each dead for another reason in turn (idx < 0, a
    NaN in x, an inf in the matched row of y) -> x (n, 3), y (m, 3), idx (n,) int64"""
    n = P + extra
    m = n + m_extra
    pairs = noisy_cloud(rng, n, np.float64)
    to = rng.permutation(m)[:n]
    y = rng.uniform(-1.0, 3.0, (m, 3))
    y[to] = pairs[:, 3:]
    x, idx = pairs[:, :3].copy(), to.astype(np.int64)
    dead = np.sort(rng.permutation(n)[:extra])
    x, y = x.astype(dtype), y.astype(dtype)
    for k, i in enumerate(dead):
        if k % 3 == 0:
            idx[i] = -1 - (k % 4)
        elif k % 3 == 1:
            x[i, k % 3] = np.nan
        else:
            y[idx[i], 1] = np.inf
    return x, y, idx


def flat_square(a, dtype):
    """four pairs whose fit at weight 1 is the identity exactly, every residual fl(a a): x on the axes of the plane z = 0, y = x -+ a z"""
    x = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], dtype=np.float64)
    y = x.copy()
    y[:, 2] = [a, a, -a, -a]
    return np.concatenate((x, y), axis=1).astype(dtype)


def half_c2_case():
    """-> (a, threshold) with 2 fl(a a) == fl(threshold threshold) exactly, a a float32: flat_square(a) then has 2 dmax exactly c2"""
    for k in range(1, 4000):
        a = 0.25 + k * 2.0 ** -12
        t0 = a * np.sqrt(2.0)
        for t in (np.nextafter(t0, 0.0), t0, np.nextafter(t0, np.inf)):
            if 2.0 * (a * a) == t * t:
                return a, float(t)
    raise AssertionError("no such pair")


def recovery_cases():
    """[(name, case dict, threshold, limit)]: the twenty runs of the table in the README (each under both losses)"""
    out = []
    for k in (300, 180):
        out += [("compat k=%d seed %d" % (k, s), cr.recovery_case(s, inliers=k), 0.05, LIMIT_COMPAT) for s in range(5)]
    for ratio in (0.4, 0.25):
        out += [("ransac %.2f seed %d" % (ratio, s), rr.recovery_case(s, inlier_ratio=ratio), 0.02, LIMIT_RANSAC) for s in range(5)]
    return out


def composition_case(seed):
    """the hard ratio: compat_ref.recovery_case(seed, inliers=60) (600 matches, 10 % right), to be pruned with
    prune_correspondences(order=2, keep=60) at threshold 0.05 before gnc_correspondences at threshold 0.05"""
    return cr.recovery_case(seed, inliers=60), 0.05, 60


def least_squares_error(case):
    keep = case["idx"] >= 0
    plain = rr.kabsch(case["x"][keep].astype(np.float64), case["y"][case["idx"][keep]].astype(np.float64))[0]
    return rr.rotation_error(plain[:9], case["C"])
