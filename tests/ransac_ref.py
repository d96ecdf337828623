"""The definition of dicp_amd.match.ransac_correspondences / correspondence_residuals in numpy, for one cloud (rules 1-6 of the docstring).

The integers (hash, sampler, counts, choice) and the residual chain in the points' dtype T are restated exactly: the residuals use the
correctly rounded fma of tests/match_ref.py for float32, and for float64 `fma64_fast`, the vectorised Boldo-Melquiond emulation
(TwoProduct, TwoSum, one addition rounded to odd, one to nearest), which tests/test_ransac_host.py holds to match_ref.fma64's exact
rational arithmetic.  The sums of a sample are restated operation by operation in double (unfused, as the host build rounds them).  The
fit itself is NOT restated: `kabsch` is the float64 numpy form (np.linalg.svd, U diag(1, 1, det) V^T) the stored poses are compared
with inside a bound, and every exact stage downstream is evaluated on the poses under test.

`wrong=` makes the deliberately wrong restatements the tests show the comparisons to refuse.  A plain module (no fixtures): the tests put
this directory on sys.path and import it.
"""
import numpy as np

from gumbel_ref import MASK, mix32
from match_ref import fma

WRONG = ("with_replacement", "mod_instead_of_mulhi", "strict_less", "unfused", "tie_high", "order_cab")
U64 = np.uint64
KAB_S0, KAB_SP, KAB_SY, KAB_M, KAB_PP, KAB_YY, NKAB = 0, 1, 4, 7, 16, 17, 18


# ------------------------------------------------------------------ float64 fma, vectorised
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma64_fast(a, b, c):
    """elementwise fma on float64 arrays: RN(th + RO(tl + ul)) with (uh, ul) = TwoProduct(a, b), (th, tl) = TwoSum(c, uh) (Boldo and
    Melquiond 2008); exact while nothing under- or overflows (|a|, |b| < 2^990), plain a b + c where an operand is not finite"""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    with np.errstate(all="ignore"):
        plain = a * b + c
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, uh)
        v, e = _two_sum(tl, ul)
        odd = (v.view(np.int64) & 1) != 0
        fix = np.isfinite(v) & (e != 0) & ~odd
        v = np.where(fix, np.nextafter(v, np.where(e > 0, np.inf, -np.inf)), v)
        z = th + v
        ok = np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(uh) & np.isfinite(z)
        return np.where(ok, z, plain)


def fma_t(a, b, c, dtype):
    return fma(a, b, c, dtype) if np.dtype(dtype) == np.float32 else fma64_fast(a, b, c)


# ------------------------------------------------------------------ rule 1
def live_mask(x, y, idx, x_rows=None):
    """(n,) bool; x (n, >=3), y (m, >=3), idx (n,) integers"""
    n, m = x.shape[0], y.shape[0]
    j = np.clip(idx, 0, m - 1)
    live = (np.arange(n) < (n if x_rows is None else int(x_rows))) & (idx >= 0)
    return live & np.isfinite(x[:, :3]).all(axis=1) & np.isfinite(y[j, :3]).all(axis=1)


def packed(x, y, idx, x_rows=None):
    """-> rows (P,) the live rows ascending, pairs (P, 6) in x's dtype"""
    rows = np.flatnonzero(live_mask(x, y, idx, x_rows))
    j = np.clip(idx[rows], 0, y.shape[0] - 1)
    return rows, np.concatenate((x[rows, :3], y[j, :3]), axis=1).astype(x.dtype)


# ------------------------------------------------------------------ rule 2
def draws(seed, cloud, H):
    """(H, 3) uint64 holding 32-bit values: u_0, u_1, u_2 of every hypothesis"""
    h = np.arange(H, dtype=U64)
    kc = mix32(U64(int(seed) & 0xFFFFFFFF) ^ ((U64(cloud) * U64(0x9E3779B9)) & MASK))
    kh = mix32(kc ^ ((h * U64(0x85EBCA6B)) & MASK))
    t = np.arange(3, dtype=U64)
    return mix32(kh[:, None] ^ ((t * U64(0xC2B2AE35) + U64(0x27D4EB2F)) & MASK)[None, :])


def positions(u, P, wrong=None):
    """u (H, 3) 32-bit draws -> (H, 3) int64: a, b, c"""
    u = np.asarray(u, dtype=U64) & MASK

    def pick(v, q):
        if wrong == "mod_instead_of_mulhi":
            return v % U64(q)
        return (v * U64(q)) >> U64(32)
    if wrong == "with_replacement":
        return np.stack([pick(u[:, t], P) for t in range(3)], axis=1).astype(np.int64)
    a = pick(u[:, 0], P).astype(np.int64)
    b = pick(u[:, 1], P - 1).astype(np.int64)
    b = b + (b >= a)
    c = pick(u[:, 2], P - 2).astype(np.int64)
    c = c + (c >= np.minimum(a, b))
    c = c + (c >= np.maximum(a, b))
    return np.stack((a, b, c), axis=1)


def samples(seed, cloud, H, P, wrong=None):
    """(H, 3) int64; -1 everywhere for P < 3"""
    if P < 3:
        return np.full((H, 3), -1, dtype=np.int64)
    return positions(draws(seed, cloud, H), P, wrong)


# ------------------------------------------------------------------ rule 3
def sums(pairs, abc, wrong=None):
    """pairs (P, 6) T, abc (H, 3) -> (H, 18) float64: the Kabsch sums, every operation rounded in double as the header writes them"""
    order = (2, 0, 1) if wrong == "order_cab" else (0, 1, 2)
    acc = np.zeros((abc.shape[0], NKAB))
    for s in order:
        row = pairs[abc[:, s]].astype(np.float64)
        p, y = row[:, :3], row[:, 3:]
        acc[:, KAB_S0] += 1.0
        for a in range(3):
            acc[:, KAB_SP + a] += p[:, a]
            acc[:, KAB_SY + a] += y[:, a]
            for b in range(3):
                acc[:, KAB_M + a * 3 + b] += y[:, a] * p[:, b]
        acc[:, KAB_PP] += (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
        acc[:, KAB_YY] += (y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2]
    return acc


def kabsch(p, y, w=None):
    """float64 reference fit of y ~ C p + r: p, y (..., k, 3), w (..., k) or None -> pose (..., 12) float64 (C row-major, r), the
    singular values (..., 3) of the centred, weighted source points, and those of the covariance W = sum w (y - my)(p - mp)^T / sum w"""
    p, y = np.asarray(p, dtype=np.float64), np.asarray(y, dtype=np.float64)
    w = np.ones(p.shape[:-1]) if w is None else np.asarray(w, dtype=np.float64)
    sw = w.sum(axis=-1)[..., None, None]
    mp = (w[..., None] * p).sum(axis=-2, keepdims=True) / sw
    my = (w[..., None] * y).sum(axis=-2, keepdims=True) / sw
    pc, yc = p - mp, y - my
    W = np.einsum("...k,...ka,...kb->...ab", w, yc, pc) / sw
    U, sw_, Vt = np.linalg.svd(W)
    d = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    d = np.where(d == 0, 1.0, d)
    D = np.zeros(U.shape)
    D[..., 0, 0] = D[..., 1, 1] = 1.0
    D[..., 2, 2] = d
    C = U @ D @ Vt
    r = my[..., 0, :] - np.einsum("...ab,...b->...a", C, mp[..., 0, :])
    sig = np.linalg.svd(np.sqrt(w)[..., None] * pc, compute_uv=False)
    return np.concatenate((C.reshape(C.shape[:-2] + (9,)), r), axis=-1), sig, sw_


# ------------------------------------------------------------------ rule 4
def residuals(poses, xs, ys, wrong=None):
    """poses (H, 12) T, xs / ys (P, 3) T -> d (H, P) T"""
    T = xs.dtype.type
    poses = np.asarray(poses, dtype=xs.dtype)
    H, P = poses.shape[0], xs.shape[0]
    d = np.zeros((H, P), dtype=xs.dtype)
    with np.errstate(all="ignore"):
        for a in range(3):
            C, r = poses[:, 3 * a:3 * a + 3], poses[:, 9 + a]
            if wrong == "unfused":
                q = np.broadcast_to(r[:, None], (H, P)).astype(T)
                for k in range(3):
                    q = (q + (C[:, k, None] * xs[None, :, k]).astype(T)).astype(T)
                e = (q - ys[None, :, a]).astype(T)
                d = (d + (e * e).astype(T)).astype(T)
            else:
                q = np.broadcast_to(r[:, None], (H, P)).astype(T)
                for k in range(3):
                    q = fma_t(C[:, k, None], xs[None, :, k], q, T).astype(T)
                e = (q - ys[None, :, a]).astype(T)
                d = fma_t(e, e, d, T).astype(T)
    return d


def thr2_of(threshold, dtype):
    return np.dtype(dtype).type(float(threshold) * float(threshold))


def inlier(d, thr2, wrong=None):
    with np.errstate(all="ignore"):
        return (d < thr2) if wrong == "strict_less" else (d <= thr2)


# ------------------------------------------------------------------ rule 5
def choose(counts, wrong=None):
    """counts (H,) -> (best, best_count): the largest count, ties to the lowest h"""
    counts = np.asarray(counts)
    top = counts.max()
    at = np.flatnonzero(counts == top)
    return int(at[-1] if wrong == "tie_high" else at[0]), int(top)


def score(poses, pairs, threshold, wrong=None):
    """poses (H, 12) T, pairs (P, 6) T -> counts (H,) int32, best, best_count; P < 3: zeros, -1, 0"""
    H = np.asarray(poses).shape[0]
    if pairs.shape[0] < 3:
        return np.zeros(H, dtype=np.int32), -1, 0
    d = residuals(poses, pairs[:, :3], pairs[:, 3:], wrong)
    counts = inlier(d, thr2_of(threshold, pairs.dtype), wrong).sum(axis=1).astype(np.int32)
    return (counts,) + choose(counts, wrong)


def residuals_rows(pose, x, y, idx, x_rows=None, wrong=None):
    """correspondence_residuals for one cloud: pose (12,) T -> d2 (n,) T, +inf on rows that are not live"""
    live = live_mask(x, y, idx, x_rows)
    out = np.full(x.shape[0], np.inf, dtype=x.dtype)
    rows = np.flatnonzero(live)
    if rows.size:
        j = np.clip(idx[rows], 0, y.shape[0] - 1)
        out[rows] = residuals(np.asarray(pose, dtype=x.dtype)[None, :], np.ascontiguousarray(x[rows, :3]), np.ascontiguousarray(y[j, :3]), wrong)[0]
    return out


IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float64)


# ------------------------------------------------------------------ rules 1-6 for one cloud
def ransac_ref(x, y, idx, threshold, hypotheses=1024, seed=0, refine=1, weight=None, x_rows=None, cloud=0, poses=None, round_poses=None):
    """-> dict: rows, pairs, P, samples (H, 3), poses (H, 12) T, counts, best, best_count, pose_best (12,) T, sets [I_0 .. I_R] (n,) bool,
    round_poses [(12,) T], inliers, pose (12,) float64 or None (the final fit on the inliers; None for fewer than one).
    poses: score these instead of the float64 fits of the samples; round_poses: the refit poses to use instead of float64 fits."""
    dt = x.dtype
    n = x.shape[0]
    rows, pairs = packed(x, y, idx, x_rows)
    P = rows.size
    H = int(hypotheses)
    abc = samples(seed, cloud, H, P)
    if poses is None:
        poses = np.tile(IDENTITY, (H, 1)) if P < 3 else kabsch(pairs[abc][:, :, :3], pairs[abc][:, :, 3:])[0]
    poses = np.asarray(poses).astype(dt)
    counts, best, best_count = score(poses, pairs, threshold)
    pose_best = poses[best] if best >= 0 else IDENTITY.astype(dt)
    thr2 = thr2_of(threshold, dt)
    some = P >= 3
    jy = np.clip(idx, 0, y.shape[0] - 1)
    w = np.ones(n) if weight is None else np.asarray(weight, dtype=np.float64)
    inl = inlier(residuals_rows(pose_best, x, y, idx, x_rows), thr2) & some
    sets, used = [inl], []
    for j in range(int(refine)):
        if round_poses is not None:
            pj = np.asarray(round_poses[j]).astype(dt)
        elif inl.any():
            pj = kabsch(x[inl, :3], y[jy[inl], :3], w[inl])[0].astype(dt)
        else:
            pj = np.full(12, np.nan, dtype=dt)
        new = inlier(residuals_rows(pj, x, y, idx, x_rows), thr2) & some
        if new.sum() >= inl.sum():
            inl = new
        sets.append(inl)
        used.append(pj)
    pose = kabsch(x[inl, :3], y[jy[inl], :3], w[inl])[0] if inl.any() else None
    return dict(rows=rows, pairs=pairs, P=P, samples=abc, poses=poses, counts=counts, best=best, best_count=best_count, pose_best=pose_best,
                sets=sets, round_poses=used, inliers=inl, pose=pose)


def rotation_error(C, C_true):
    """the angle of C C_true^T, radians"""
    R = np.asarray(C, dtype=np.float64).reshape(3, 3) @ np.asarray(C_true, dtype=np.float64).reshape(3, 3).T
    return float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))


# ------------------------------------------------------------------ inputs the CPU and the GPU tests share
def rotation(rng, angle=None):
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    th = rng.uniform(0.2, 1.0) if angle is None else angle
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def chain_case(seed):
    """match_cases.end_to_end (descriptors whose accepted matches are exactly gt) plus the corruption of half of the matches: the corrupted
    rows name the row of y nearest to R_bad x + t_bad, a second rigid motion 2.5 rad away -- structured outliers, which drag the fit over
    every match about a radian off (uniformly random ones would average out of a Procrustes fit).
    -> end_to_end's dict with corrupt(idx) -> the corrupted copy of an accepted-match vector, bad (rows), threshold"""
    import match_cases as mc
    c = mc.end_to_end(seed=seed)
    rng = np.random.default_rng(50 + seed)
    live = np.flatnonzero(c["gt"] >= 0)
    bad = rng.permutation(live)[:live.size // 2]
    Rb, tb = mc.rotation(2.5, [1.0, 0.2, -0.4]), np.array([0.1, 0.0, -0.1])
    xb = c["x"][bad].astype(np.float64) @ Rb.T + tb
    to = np.argmin(((xb[:, None, :] - c["y"][None].astype(np.float64)) ** 2).sum(-1), axis=1)

    def corrupt(idx):
        out = np.array(idx, dtype=np.int64, copy=True)
        out[bad] = to
        return out
    return dict(c, corrupt=corrupt, bad=bad, threshold=0.02)


def recovery_case(seed, n=300, inlier_ratio=0.4, noise=0.005, dtype=np.float32):
    """x (n, 3) uniform in [-1, 1]^3; y = C x + r + noise for the first inliers (shuffled), uniform in [-2, 2]^3 for the rest; idx a
    permutation -> dict x, y, idx, truth (n,) bool, C (3, 3), r (3,)"""
    rng = np.random.default_rng(1000 + seed)
    C, r = rotation(rng), rng.uniform(-0.5, 0.5, 3)
    x = rng.uniform(-1, 1, (n, 3))
    truth = np.zeros(n, dtype=bool)
    truth[rng.permutation(n)[:int(round(inlier_ratio * n))]] = True
    yi = x @ C.T + r + noise * rng.standard_normal((n, 3))
    yi[~truth] = rng.uniform(-2, 2, (int((~truth).sum()), 3))
    perm = rng.permutation(n)
    y = np.empty_like(yi)
    y[perm] = yi
    return dict(x=x.astype(dtype), y=y.astype(dtype), idx=perm.astype(np.int64), truth=truth, C=C, r=r)
