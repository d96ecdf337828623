"""A float64 restatement of the Gauss-Newton step kernels (dicp_step / dicp_step_bwd / dicp_loop_init), written from include/dicp_hip.h's
description of dicp_step_io and dicp_step_bwd and from the reference loop ICP.py:198-260 as quoted there.  numpy (and torch on the CPU for the
adjoint); no GPU, no library.  Every model takes `wrong=`: a deliberately wrong rule, so that tests/test_step_ref.py can show the comparators
refusing it.

Error model (u = 2^-53, the unit roundoff of the double arithmetic both sides work in; ulp_T = spacing of the cloud type T):

  sums      the partials are T values, added in double in a fixed order (even blocks in order, odd blocks in order, then the two): the model
            adds in the same order, so cost, n_matched and areg = A + 1e-12 I are held BIT FOR BIT.
  delta     both sides solve Areg x = b by Gaussian elimination with partial pivoting.  Wilkinson's backward error (Higham, Accuracy and
            Stability, Thm 9.5): (A + dA) x^ = b with |dA|_inf <= n^2 gamma_3n rho |A|_inf, gamma_k = k u / (1 - k u), rho = the growth factor
            (taken from ge_growth, this file's own elimination).  Forward: |x - x^|_inf <= eps kappa_inf |x|_inf / (1 - eps kappa_inf), eps =
            n^2 gamma_3n rho.  Counted TWICE (the reference is a float64 solve too), plus 0.5 ulp_T(delta_ref) for the rounding to T.  Factor 1.
  pose      recomputed from the kernel's OWN stored delta: R = exp(delta^) costs a square root, one sin and one cos (1 ulp each allowed) and at
            most a dozen further roundings of quantities <= 2 per entry: |dR| <= 32 u per entry and per side; C' = R^T C adds gamma_3 sum|R||C|.
            Bound per entry: (2 * 32 + 6) u sum_k |C_kj| + 0.5 ulp_T.  r' = r - delta[3:] is ONE double subtraction rounded to T: bit for bit.
  residual  (ill-conditioned systems) |Areg delta + b|_inf <= eps |A|_inf |delta|_inf (backward error) + |A|_inf 0.5 ulp_T(delta) (the
            stored step is rounded to T) + gamma_8 (|A||delta| + |b|) (this evaluation).
  adjoint   g = Areg^-1 gd: the solve bound above on the adjoint system plus |Areg^-1|_inf |d gd|_inf, d gd = the rounding of gd (64 u times
            its magnitude 18 max|C| max|gC'| (1 + |phi|^2) + |gr'|_inf, per side); gb = -g, Gs_ij = -(g_i delta_j + delta_i g_j) multiplies
            it by |delta_i| + |delta_j| and adds 3 u |Gs_ij|; 0.5 ulp_T for the stores.  The model's autograd multiplies g by ITS OWN solve of
            b = -Areg delta where the kernel multiplies by the stored delta: twice the forward bound of that solve times |g_i| + |g_j| more.
            gC = R gC': (2 * 32 + 6) u sum_k |gC'_kj|.
"""
from fractions import Fraction

import numpy as np

ACC_A, ACC_B, ACC_COST, ACC_SUMW, ACC_NMATCH, NACC, NACC_PAD = 0, 21, 27, 28, 29, 30, 32
NBWD, NBWD_PAD = 12, 16
CERT_OFF_FOR_GOOD, CERT_RECERTIFY = 1 << 20, -2
U64 = 2.0 ** -53
EXP_U = 32.0            # |dR| per entry of exp(delta^), in u (see above)


def rT(x, T):
    """x rounded to T, as float64"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float64).astype(T).astype(np.float64)


def ulp(x, T):
    """spacing of T at |x| (of the smallest normal below it)"""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), float(np.finfo(T).tiny)).astype(T)
    return np.spacing(a).astype(np.float64)


def fma(a, b, c, T):
    """a b + c rounded ONCE to T (exact rational arithmetic)"""
    f = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    d = f.numerator / f.denominator                   # correctly rounded to double
    if T == np.float64:
        return d
    g = np.float32(d)                                 # (double rounding can be one float32 off: take the nearest of the three)
    cands = [g, np.nextafter(g, np.float32(np.inf)), np.nextafter(g, np.float32(-np.inf))]
    return float(min(cands, key=lambda v: (abs(Fraction(float(v)) - f), v != g)))


# ------------------------------------------------------------------ sums
def ordered_sums(partials, wrong=None):
    """(nblk, S) T -> (S,) double: even blocks in order, plus odd blocks in order"""
    p = np.asarray(partials).astype(np.float64)
    nblk = p.shape[0] - (1 if wrong == "drop_last_block" else 0)
    e, o = np.zeros(p.shape[1]), np.zeros(p.shape[1])
    with np.errstate(over="ignore", invalid="ignore"):      # (the pad slots may hold anything)
        for b in range(0, nblk, 2):
            e = e + p[b]
        for b in range(1, nblk, 2):
            o = o + p[b]
        return e + o


def sums4(partials):
    """(nblk, S) T -> (S,) double: (part0 + part2) + (part1 + part3), part p = blocks p, p + 4, .. in order"""
    p = np.asarray(partials).astype(np.float64)
    part = [np.zeros(p.shape[1]) for _ in range(4)]
    for b in range(p.shape[0]):
        part[b % 4] = part[b % 4] + p[b]
    return (part[0] + part[2]) + (part[1] + part[3])


def sym6(tri21):
    A = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = tri21[k]
            k += 1
    return A


def tri21(A):
    return np.array([A[i, j] for i in range(6) for j in range(i, 6)])


def slots(dim, wrong=None):
    if dim == 2:
        return [0, 1, 2] if wrong == "dim2_slots_0_3" else [2, 3, 4]
    return list(range(6))


# ------------------------------------------------------------------ the solve and its error bound
def ge_growth(A):
    """Gaussian elimination with partial pivoting on a copy of A: the growth factor max_k max|a_ij^(k)| / max|a_ij| -- None when a pivot is
    exactly zero (the kernels then leave the step at zero)"""
    M = np.array(A, dtype=np.float64)
    n = M.shape[0]
    top = big = np.abs(M).max()
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if M[p, k] == 0.0:
            return None
        M[[k, p]] = M[[p, k]]
        M[k + 1:, k + 1:] -= np.outer(M[k + 1:, k] / M[k, k], M[k, k + 1:])
        M[k + 1:, k] = 0.0
        big = max(big, np.abs(M[k + 1:, k + 1:]).max() if k + 1 < n else 0.0)
    return big / top if top > 0 else 1.0


def backward_eps(A):
    """eps with (A + dA) x^ = b, |dA|_inf <= eps |A|_inf"""
    n = A.shape[0]
    g = 3 * n * U64 / (1 - 3 * n * U64)
    return n * n * g * ge_growth(A)


def solve_bound(A, x):
    """|x - x^|_inf for one elimination of A x = b (inf when the bound's denominator is gone)"""
    ek = backward_eps(A) * np.linalg.cond(A, np.inf)
    return np.inf if ek >= 1 else ek * np.abs(x).max() / (1 - ek)


def so3_exp(phi):
    """exp(phi^) = I + a K + b K^2, a = sin t / t, b = 2 sin^2(t/2) / t^2 -- np.sinc is exact at 0: no branch"""
    x, y, z = (float(v) for v in phi[:3])
    t = np.sqrt(x * x + y * y + z * z)
    a = np.sinc(t / np.pi)
    b = 0.5 * np.sinc(t / (2 * np.pi)) ** 2
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + a * K + b * (K @ K)


def frame_pose(frame, pose, T):
    """[Q C | Q r + t] in T: what the next search reads.  No frame: the pose; Q == I exactly: the plain addition r + t; else every entry one chain
    of fused multiply-adds, innermost term first: Q_i0 C_0j + (Q_i1 C_1j + Q_i2 C_2j), Q_i0 r_0 + (Q_i1 r_1 + (Q_i2 r_2 + t_i))"""
    pose = rT(pose, T)
    if frame is None:
        return pose.copy()
    F = rT(frame, T)
    out = pose.copy()
    if np.array_equal(F[:9], np.eye(3).ravel()):
        out[9:] = rT(pose[9:] + F[9:], T)
        return out
    for i in range(3):
        for j in range(3):
            out[3 * i + j] = fma(F[3 * i], pose[j], fma(F[3 * i + 1], pose[3 + j], rT(F[3 * i + 2] * pose[6 + j], T), T), T)
        out[9 + i] = fma(F[3 * i], pose[9], fma(F[3 * i + 1], pose[10], fma(F[3 * i + 2], pose[11], F[9 + i], T), T), T)
    return out


def apply_delta(pose, d6, T, wrong=None):
    """pose_out = round_T(exp(d^)^T C, r - d[3:])"""
    C, r = np.asarray(pose[:9], dtype=np.float64).reshape(3, 3), np.asarray(pose[9:], dtype=np.float64)
    R = so3_exp(d6)
    Cn = (R if wrong == "R_not_RT" else R.T) @ C
    rn = r + d6[3:] if wrong == "r_plus" else r - d6[3:]
    return rT(np.concatenate([Cn.ravel(), rn]), T)


# ------------------------------------------------------------------ dicp_step, one cloud
def step_model(partials, io, wrong=None):
    """partials (nblk, 32) T; io: T, dim, iter, const_iter, tolerance, pose_in (12), cost_prev (None | number), alive, converged, iterations,
    matched_ratio, n_start, weights (w_cur and w_prev both given), w_copied, frame (None | 12) -> every output of dicp_step for the cloud"""
    T = io["T"]
    s = ordered_sums(partials, wrong)
    A, b = sym6(s[ACC_A:ACC_A + 21]), s[ACC_B:ACC_B + 6]
    sl = slots(io["dim"], wrong)
    D = len(sl)
    Ar = A[np.ix_(sl, sl)] + 1e-12 * np.eye(D)
    areg = np.zeros((6, 6))
    areg[:D, :D] = Ar                                   # compact, leading dimension 6
    exact = np.zeros(6)
    if ge_growth(Ar) is not None:
        exact[sl] = -np.linalg.solve(Ar, b[sl])
    d6 = exact if wrong == "unrounded_delta" else rT(exact, T)
    pose_out = apply_delta(rT(io["pose_in"], T), d6, T, wrong)
    cost = float(rT(s[ACC_COST], T))
    if io.get("cost_prev") is not None and cost == 0.0:
        cost = float(rT(io["cost_prev"], T))
    nmatch = s[ACC_NMATCH]
    hit = bool(float(rT(np.sqrt(np.sum(rT(exact, T) ** 2)), T)) < io["tolerance"])
    alive_in = float(rT(io["alive"], T))
    out = {"sums": s, "areg": areg.ravel(), "delta": rT(exact, T), "delta_exact": exact, "delta_applied": d6, "pose_out": pose_out, "cost": cost,
           "n_matched": float(rT(nmatch, T)), "hit": hit, "converged": 1 if hit else int(io["converged"]), "not_converged": 0 if hit else 1,
           "iterations": float(io["iterations"]), "matched_ratio": float(io["matched_ratio"]), "alive_out": alive_in}
    if hit and not io["const_iter"]:
        if out["iterations"] == 0.0:
            out["iterations"] = float(io["iter"] + 1)
        if out["matched_ratio"] == 0.0:
            start = np.float32(rT(io["n_start"], T)) if alive_in != 0.0 else np.float32(0)
            if start == 0:
                start = np.float32(1)
            out["matched_ratio"] = float(rT(np.float32(nmatch) / start, T))     # one float32 division
        out["alive_out"] = 0.0
    out["copy"] = bool(io.get("weights") and s[ACC_SUMW] == 0.0 and not (io.get("w_copied") and alive_in == 0.0))
    out["pose_search_out"] = frame_pose(io.get("frame"), pose_out, T)
    return out


def pose_from_delta_bound(pose_in, T):
    """per entry of C': the float64 operation-count bound + 0.5 ulp_T is added by the caller"""
    C = np.abs(rT(pose_in[:9], T).reshape(3, 3))
    return np.repeat(((2 * EXP_U + 6) * U64 * C.sum(0))[None, :], 3, 0).ravel()


def hold_forward(got, partials, io, ill=False):
    """got: the kernel's (or a wrong variant's) outputs for one cloud -> {family: (ok, |error| / bound)}"""
    T = io["T"]
    ref = step_model(partials, io)
    res = {}

    def exact(name, a, b):
        res[name] = (bool(np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))), 0.0)

    def within(name, err, bound):
        err, bound = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(bound, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        res[name] = (bool(np.all(err <= bound)) and bool(np.all(np.isfinite(err))), float(np.max(ratio)))

    exact("cost", got["cost"], ref["cost"])
    exact("n_matched", got["n_matched"], ref["n_matched"])
    exact("areg", got["areg"], ref["areg"])
    sl = slots(io["dim"])
    D = len(sl)
    Ar = ref["areg"].reshape(6, 6)[:D, :D]
    b = ref["sums"][ACC_B:ACC_B + 6][sl]
    gd = np.asarray(got["delta"], dtype=np.float64)
    exact("delta_off_slots", gd[[i for i in range(6) if i not in sl]], np.zeros(6 - D))
    if ill:
        eps = backward_eps(Ar)
        an, bn = np.abs(Ar).sum(1).max(), np.abs(gd[sl]).max()
        bound = eps * an * bn + an * 0.5 * ulp(gd[sl], T).max() + 8 * U64 / (1 - 8 * U64) * (np.abs(Ar) @ np.abs(gd[sl]) + np.abs(b))
        within("residual", Ar @ gd[sl] + b, bound)
        res["finite"] = (bool(np.all(np.isfinite(gd)) and np.all(np.isfinite(got["pose_out"]))), 0.0)
    else:
        within("delta", gd - ref["delta_exact"], 0.5 * ulp(ref["delta_exact"], T) + 2 * solve_bound(Ar, ref["delta_exact"][sl]))
    mine = apply_delta(rT(io["pose_in"], T), gd, T)            # from the kernel's OWN stored delta
    full = apply_delta(rT(io["pose_in"], T), gd, np.float64)
    within("pose_C", np.asarray(got["pose_out"][:9], dtype=np.float64) - full[:9], 0.5 * ulp(full[:9], T) + pose_from_delta_bound(io["pose_in"], T))
    exact("pose_r", got["pose_out"][9:], mine[9:])
    return res


# ------------------------------------------------------------------ dicp_step_bwd, one cloud
def _exp_torch(phi):
    import torch
    t2 = (phi * phi).sum()
    if float(t2.detach()) < 1e-8:        # (the derivative of sqrt at 0: the series in t^2 instead)
        a = 1 - t2 / 6 + t2 * t2 / 120
        b = 0.5 - t2 / 24 + t2 * t2 / 720
    else:
        t = torch.sqrt(t2)
        a, b = torch.sin(t) / t, (1 - torch.cos(t)) / t2
    z = torch.zeros((), dtype=phi.dtype)
    K = torch.stack([torch.stack([z, -phi[2], phi[1]]), torch.stack([phi[2], z, -phi[0]]), torch.stack([-phi[1], phi[0], z])])
    return torch.eye(3, dtype=phi.dtype) + a * K + b * (K @ K)


def step_bwd_model(gpose_in, bwd_partials, dim, pose_k, delta_k, areg, route="model", wrong=None):
    """float64 autograd through delta = -solve(Areg, b) -> C' = exp(delta^)^T C, r' = r - delta[3:], with b chosen so that the solve returns
    delta_k.  The incoming cotangent is gpose_in + the reduced bwd_partials.  -> Gs (36) = G_A + G_A^T at the optimised slots, gb (6), gpose (12),
    and g (12) the cotangent that went in.  route "second": explicit inverse + torch.matrix_exp."""
    import torch
    g = np.asarray(gpose_in, dtype=np.float64).copy()
    if bwd_partials is not None:
        g = sums4(np.asarray(bwd_partials)[:, :NBWD]) + g
    sl = slots(dim)
    D = len(sl)
    Ar = np.asarray(areg, dtype=np.float64).reshape(6, 6)[:D, :D]
    d = np.asarray(delta_k, dtype=np.float64)
    Gs, gb = np.zeros((6, 6)), np.zeros(6)
    singular = ge_growth(Ar) is None
    At = torch.tensor(np.eye(D) if singular else Ar, requires_grad=True)
    bt = torch.tensor(-(np.eye(D) if singular else Ar) @ d[sl], requires_grad=True)
    Ct = torch.tensor(np.asarray(pose_k[:9], dtype=np.float64).reshape(3, 3), requires_grad=True)
    rt = torch.tensor(np.zeros(3), requires_grad=True)
    if route == "second":
        dsub = -(torch.linalg.inv(At) @ bt)
    else:
        dsub = -torch.linalg.solve(At, bt)
    # (the kernel applies the STORED delta: the values are delta_k's, the derivative the solve's)
    dsub = dsub + (torch.tensor(d[sl]) - dsub).detach()
    full = torch.zeros(6, dtype=torch.float64)
    full = full.index_put((torch.tensor(sl),), dsub) + torch.tensor(np.where(np.isin(np.arange(6), sl), 0.0, d))
    if route == "second":
        z = torch.zeros((), dtype=torch.float64)
        K = torch.stack([torch.stack([z, -full[2], full[1]]), torch.stack([full[2], z, -full[0]]), torch.stack([-full[1], full[0], z])])
        R = torch.matrix_exp(K)
    else:
        R = _exp_torch(full[:3])
    Cn, rn = R.T @ Ct, rt - full[3:]
    ((Cn * torch.tensor(g[:9].reshape(3, 3))).sum() + (rn * torch.tensor(g[9:])).sum()).backward()
    if not singular:
        GA = At.grad.numpy()
        Gs[np.ix_(sl, sl)] = GA if wrong == "no_transpose_half" else GA + GA.T
        gb[sl] = bt.grad.numpy()
    return {"gs": Gs.ravel(), "gb": gb, "gpose": np.concatenate([Ct.grad.numpy().ravel(), rt.grad.numpy()]), "g": g}


def hold_backward(got, gpose_in, bwd_partials, dim, pose_k, delta_k, areg, T):
    """got: gs (36), gb (6), gpose (12) of one cloud -> {family: (ok, |error| / bound)}"""
    ref = step_bwd_model(gpose_in, bwd_partials, dim, pose_k, delta_k, areg)
    res = {}
    g = ref["g"]
    sl = slots(dim)
    D = len(sl)
    d = np.asarray(delta_k, dtype=np.float64)
    Ar = np.asarray(areg, dtype=np.float64).reshape(6, 6)[:D, :D]

    def within(name, err, bound):
        err, bound = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(bound, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        res[name] = (bool(np.all(err <= bound)) and bool(np.all(np.isfinite(err))), float(np.max(ratio)))

    gp = np.asarray(got["gpose"], dtype=np.float64)
    res["gr"] = (bool(np.array_equal(gp[9:], g[9:])), 0.0)
    gCn = np.abs(g[:9].reshape(3, 3))
    within("gC", gp[:9] - ref["gpose"][:9], np.repeat(((2 * EXP_U + 6) * U64 * gCn.sum(0))[None, :], 3, 0).ravel())
    gs, gb = np.asarray(got["gs"], dtype=np.float64).reshape(6, 6), np.asarray(got["gb"], dtype=np.float64)
    off = np.ones((6, 6), dtype=bool)
    off[np.ix_(sl, sl)] = False
    res["off_slots"] = (bool(np.all(gs[off] == 0) and np.all(gb[[i for i in range(6) if i not in sl]] == 0)), 0.0)
    if ge_growth(Ar) is None:
        res["singular"] = (bool(np.all(gs == 0) and np.all(gb == 0)), 0.0)
        return res
    gvec = -ref["gb"][sl]                                # g = Areg^-1 gd
    mag = 18 * np.abs(pose_k[:9]).max() * np.abs(g[:9]).max() * (1 + float(np.sum(d[:3] ** 2))) + np.abs(g[9:]).max()
    Eg = 2 * (solve_bound(Ar, gvec) + np.abs(np.linalg.inv(Ar)).sum(1).max() * 64 * U64 * mag)
    within("gb", gb[sl] - ref["gb"][sl], 0.5 * ulp(ref["gb"][sl], T) + Eg)
    ad = np.abs(d[sl])
    Gref = ref["gs"].reshape(6, 6)[np.ix_(sl, sl)]
    Ed = 2 * solve_bound(Ar, d[sl])                     # (autograd multiplies g by ITS solve of b = -Areg delta, the kernel by the stored delta)
    ag = np.abs(gvec)
    within("gs", gs[np.ix_(sl, sl)] - Gref, 0.5 * ulp(Gref, T) + Eg * (ad[:, None] + ad[None, :]) + Ed * (ag[:, None] + ag[None, :]) + 3 * U64 * np.abs(Gref))
    return res


# ------------------------------------------------------------------ the truncated reverse sweep's verdict
def skip_model(Gs, gb, areg, deltas_before, dim, alive, ended, mref, eps):
    """-> (verdict, mref', live): 1 = not alive at this iteration, 2 = the sweep ends here (sticky), 0 = takes part.
    m = max(max_ab |G_ab| s_a s_b, max_a |g_a| s_a), s_a = sqrt(A_aa); w = max_a |g_a| s_a x max_{k' < k, b} |delta_k',b| s_b;
    ends when 16 max(m, w) <= eps mref; a NaN measure never ends a sweep; mref is raised only when m > mref; live counts verdict 0."""
    if ended:
        return 2, mref, 0
    if not alive:
        return 1, mref, 0
    sl = slots(dim)
    D = len(sl)
    s = np.sqrt(np.abs(np.diag(np.asarray(areg, dtype=np.float64).reshape(6, 6))[:D]))
    G = np.abs(np.asarray(Gs, dtype=np.float64).reshape(6, 6)[np.ix_(sl, sl)]) * s[:, None] * s[None, :]
    gv = np.abs(np.asarray(gb, dtype=np.float64)[sl]) * s
    db = np.asarray(deltas_before, dtype=np.float64).reshape(-1, 6)
    amp = (np.abs(db[:, sl]).max(0) * s) if db.shape[0] else np.zeros(D)
    if np.isnan(G).any() or np.isnan(gv).any() or np.isnan(amp).any():
        return 0, mref, 1
    m = max(G.max(), gv.max())
    worst = max(m, gv.max() * amp.max())
    if 16.0 * worst <= eps * mref:
        return 2, mref, 0
    return 0, (m if m > mref else mref), 1


# ------------------------------------------------------------------ match certificates: motion bound, work lists, per-cloud switch
def cert_ulp(T):
    """the constant the certificates call one ulp of T (a T value in T arithmetic, a double in the step's double arithmetic)"""
    return 1.2e-7 if T == np.float32 else 2.3e-16


def rmax_model(src, T):
    """(radius, midpoint) of the cloud's bounding box, in T: 0.5 |hi - lo| (1 + 8 ulp) + 8 ulp |mid|"""
    p = np.asarray(src, dtype=T)
    lo, hi = p.min(0), p.max(0)
    mid = (T(0.5) * (lo + hi)).astype(T)
    u8 = T(8) * T(cert_ulp(T))
    d2, pn = T(0), T(0)
    for k in range(3):
        d2 = T(d2 + T((hi[k] - lo[k]) * (hi[k] - lo[k])))
        pn = T(pn + T(mid[k] * mid[k]))
    rad = T(T(T(T(0.5) * np.sqrt(d2)) * T(T(1) + u8)) + T(u8 * np.sqrt(pn)))
    return np.array([rad, mid[0], mid[1], mid[2]], dtype=np.float64)


def motion_model(poses, rmax, frame, T, factor=1.0001, radius_term=True, p0_term=True, e_ulps=8.0):
    """poses (K + 1, 12) T, rmax (4) -> (K + 1, 2): M_0 = 0, M_k+1 = round_up_T(M_k + (|dC|_F radius + |dC p0 + dr|) factor), the sum in double;
    e_k = round_T(e_ulps ulp (|p0| + radius + |r_k| + |t| + 1) factor) (factor 1 for e_0, which is made in T by dicp_loop_init)."""
    poses = rT(poses, T)
    rad, p0 = float(rmax[0]), np.asarray(rmax[1:4], dtype=np.float64)
    cn = 0.0 if frame is None else float(np.sqrt(np.sum(rT(frame, T)[9:] ** 2)))
    ul = cert_ulp(T)
    out = np.zeros((poses.shape[0], 2))
    pn0, rn0 = np.sqrt(T(np.sum(p0.astype(T) ** 2))), np.sqrt(T(np.sum(poses[0, 9:].astype(T) ** 2)))
    out[0, 1] = float(T(T(e_ulps) * T(ul)) * T(T(T(T(T(pn0) + T(rad)) + T(rn0)) + T(cn)) + T(1)))
    for k in range(1, poses.shape[0]):
        dC = (poses[k, :9] - poses[k - 1, :9]).reshape(3, 3)
        dr = poses[k, 9:] - poses[k - 1, 9:]
        mv = dr + (dC @ p0 if p0_term else 0.0)
        step = ((np.sqrt(np.sum(dC * dC)) * rad if radius_term else 0.0) + np.sqrt(np.sum(mv * mv))) * factor
        nxt = float(rT(out[k - 1, 0] + step, T))
        out[k, 0] = float(rT(nxt + abs(nxt) * float(rT(4.0 * ul, T)), T))
        out[k, 1] = float(rT(e_ulps * ul * (np.sqrt(np.sum(p0 * p0)) + rad + np.sqrt(np.sum(poses[k, 9:] ** 2)) + cn + 1.0) * factor, T))
    return out


def motion_check(points, poses, poses_search, dcum, T):
    """The two claims the match certificates rest on, for every point p and every pair j < k, with NO tolerance:
         world   |pose_k p - pose_j p| <= M_k - M_j
         search  |ps_k p - ps_j p| + rho_j(p) + rho_k(p) <= (M_k - M_j) + e_j + e_k
       The stored T values are exact reals; both sides are evaluated one precision up (float64 / np.longdouble) and the left side is lowered by
       that evaluation's own rounding.  rho = the worst rounding of a 3-term dot product plus add evaluated in T in any order, with or without fma:
       per component 4u / (1 - 4u) (sum_j |ps_ij p_j| + |ps_r,i|), as a 2-norm.  -> (largest lhs / rhs world, search; 0 / 0 counts as 0)"""
    H = np.float64 if T == np.float32 else np.longdouble
    uh = H(np.finfo(H).eps) / 2
    u = H(np.finfo(T).eps) / 2
    p = np.asarray(points).astype(T).astype(H)
    P, S, D = (np.asarray(a).astype(T).astype(H) for a in (poses, poses_search, dcum))
    ap = np.abs(p)

    def rho(ps):
        mag = ap @ np.abs(ps[:9].reshape(3, 3)).T + np.abs(ps[9:])
        return np.sqrt(np.sum((4 * u / (1 - 4 * u) * mag) ** 2, axis=1))

    def moved(a, b):
        dC, dr = (b[:9] - a[:9]).reshape(3, 3), b[9:] - a[9:]
        d = p @ dC.T + dr
        lhs = np.sqrt(np.sum(d * d, axis=1))
        own = np.sqrt(np.sum((8 * uh * (ap @ np.abs(dC).T + np.abs(dr))) ** 2, axis=1)) + 4 * uh * lhs
        return lhs - own

    worst = [H(0), H(0)]
    rhos = [rho(S[k]) for k in range(P.shape[0])]
    for k in range(P.shape[0]):
        for j in range(k):
            dM = D[k, 0] - D[j, 0]
            for which, lhs, rhs in ((0, moved(P[j], P[k]), dM), (1, moved(S[j], S[k]) + rhos[j] + rhos[k], dM + D[j, 1] + D[k, 1])):
                lhs = np.maximum(lhs, 0)
                top = lhs.max()
                ratio = H(0) if top == 0 else (H(np.inf) if rhs <= 0 else top / rhs)
                worst[which] = max(worst[which], ratio)
    return float(worst[0]), float(worst[1])


def cert_spent(M, e, T):
    """what a budget is compared with: (M + e)(1 + 8 ulp), in T"""
    return float(T(T(T(M) + T(e)) * T(T(1) + T(8) * T(cert_ulp(T)))))


def cert_state_model(cc, n):
    """cc (8) int32 of one cloud: [0] units / [1] single queries searched again in this iteration, [2] the state (0 on, -1 on with one strike,
    k > 0 off for k more iterations, CERT_OFF_FOR_GOOD, CERT_RECERTIFY), [3] the cloud's units (0: no certified iteration ran -- nothing changes),
    [4] the last back-off length, [5] candidate sets are kept, [6] queries that came back without a certificate, [7] iterations that did not pay.
    -> (cc', next state).  Certificates that cost more than 60 % of a full search (a unit searched again 1.3, a single query 0.12 of a unit) are
    switched off -- for good where the evidence is structural, for 2, 4, .. 16 iterations and then certified afresh where a guarded iteration
    was costly twice in a row."""
    cc = [int(v) for v in cc]
    c_units, c_single, state, units, c_back, sets, nocert = cc[0], cc[1], cc[2], cc[3], cc[4], cc[5] != 0, cc[6]
    if units <= 0:
        return cc, state
    costly = 1.3 * c_units + 0.12 * c_single > 0.6 * units
    if state >= CERT_OFF_FOR_GOOD:
        nxt = state
    elif state > 0:                                     # off for a while: count down, then one iteration that certifies afresh
        nxt = state - 1 if state > 1 else CERT_RECERTIFY
    elif state == CERT_RECERTIFY:
        nxt = (-1 if costly else 0) if sets else (CERT_OFF_FOR_GOOD if 0.12 * c_single > 0.6 * units else 0)
    elif sets and 2 * nocert > n:                       # most queries without a certificate: not worth the sets
        nxt = CERT_OFF_FOR_GOOD
    elif not costly:
        nxt = 0
    elif c_units == 0 and (not sets or state == -1):    # costly by per-query work alone: structural
        nxt = CERT_OFF_FOR_GOOD
    elif state == -1:                                   # second strike in a row: back off, doubling
        nxt = min(2 * c_back, 16) if c_back > 0 else 2
        cc[4] = nxt
    else:
        nxt = -1
    cc[2] = nxt
    if costly or state > 0:
        cc[7] += 1
    cc[0] = cc[1] = cc[3] = cc[6] = 0
    return cc, nxt


def guard_list_model(cloud, qu, spent, state, units, have=None, n=0):
    """The entries the next guard launch must see for one cloud (list = cloud & 7): every unit whose filter value does not stand STRICTLY above
    `spent` (equal, below, negative marks and NaN all mean work), or all units when the certificates are off or tried again; with candidate-set
    lists (have = the list's length) one entry -1 - (cloud ceil(n/64) + c) per chunk of 64 while the certificates are on.
    -> (sorted entries, scount', filled-to) -- scount' None: unchanged"""
    on = state <= 0 and state != CERT_RECERTIFY
    ent = [cloud * units + u for u in range(units) if not (on and qu[u] >= 0 and qu[u] > spent)]
    scount, upto = None, None
    if have is not None:
        if not on:
            scount = 0
        else:
            have = min(int(have), n)
            nch = (have + 63) // 64
            if nch:
                upto = min(nch * 64, n)
                if upto > have:
                    scount = upto
                ent += [-1 - (cloud * ((n + 63) // 64) + c) for c in range(nch)]
    return sorted(ent), scount, upto


# ------------------------------------------------------------------ inputs (shared by the CPU and the GPU tests)
ANGLES = (0.0, 1e-9, 1e-4 * (1 - 1e-3), 1e-4 * (1 + 1e-3), 1e-3, 0.3, 3.0)       # |phi|^2 = 1e-8 is where exp(phi^) changes form
KAPPAS = {np.float32: (1e1, 1e3, 1e4), np.float64: (1e1, 1e3, 1e6)}              # (64 float32 blocks round the sums by ~1e-5 |A|: no matrix beyond 1e4 survives that)


def spd(rng, D, kappa, scale=1.0):
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    return (Q * (scale * np.logspace(0, -np.log10(kappa), D))) @ Q.T


def delta_star(rng, angle, trans, dim):
    d = np.zeros(6)
    if dim == 2:
        d[2] = angle
        d[3:5] = rng.normal(size=2)
        d[3:5] *= trans / max(np.abs(d[3:5]).max(), 1e-300)
    else:
        ax = rng.normal(size=3)
        d[:3] = angle * ax / np.linalg.norm(ax)
        d[3:] = rng.normal(size=3)
        d[3:] *= trans / np.abs(d[3:]).max()
    return d


def split_blocks(rng, total, nblk, T, integer_slots=(ACC_NMATCH,)):
    """total (S,) -> (nblk, S) T whose sum is total up to T's rounding: mixed signs and magnitudes (integers where the sum must stay one)"""
    S = total.shape[0]
    parts = rng.normal(size=(nblk, S)) * 10.0 ** rng.uniform(-2, 1, size=(nblk, 1)) * np.maximum(np.abs(total), 1e-3)[None, :]
    for s in integer_slots:
        parts[:, s] = rng.randint(-40, 40, size=nblk)
    parts[0] += total - parts.sum(0)
    return parts.astype(T)


def make_partials(rng, nblk, T, dim, dstar, kappa, garbage=True, cost=None, sumw=7.5, nmatch=33.0):
    """one cloud's (nblk, 32) partials: A SPD with condition `kappa` (the full 6 x 6; dim 2 reads slots 2:5 of it), b = -A delta* on the
    optimised slots (anything elsewhere), slots 30 and 31 garbage"""
    A = spd(rng, 6, kappa, scale=10.0 ** rng.uniform(-1, 2))
    sl = slots(dim)
    if dim == 2:                                        # (the condition number promised is the sub-block's)
        A[np.ix_(sl, sl)] = spd(rng, 3, kappa, scale=np.abs(A).max())
    b = rng.normal(size=6)
    b[sl] = -A[np.ix_(sl, sl)] @ dstar[sl]
    total = np.zeros(NACC_PAD)
    total[ACC_A:ACC_A + 21], total[ACC_B:ACC_B + 6] = tri21(A), b
    total[ACC_COST], total[ACC_SUMW], total[ACC_NMATCH] = (rng.uniform(0.1, 5.0) if cost is None else cost), sumw, nmatch
    p = split_blocks(rng, total, nblk, T)
    if garbage:
        p[:, 30] = np.nan
        p[:, 31] = T(np.finfo(T).max)
    return p


def ill_partials(rng, kind, T):
    """(3, 32) partials of systems only the 1e-12 regulariser keeps from singular: point-to-plane rows j = [p x n, n], b = sum j e"""
    tot = np.zeros(NACC_PAD)
    if kind != "zeros":
        npts = 1 if kind == "one_point" else 40
        p = rng.normal(size=(npts, 3)) * 3
        nrm = np.tile([0.0, 0.0, 1.0], (npts, 1)) if kind == "planar" else rng.normal(size=(npts, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        J = np.concatenate([np.cross(p, nrm), nrm], axis=1)
        e = rng.normal(size=npts) * 0.1
        tot[ACC_A:ACC_A + 21], tot[ACC_B:ACC_B + 6] = tri21(J.T @ J), J.T @ e
        tot[ACC_COST], tot[ACC_SUMW], tot[ACC_NMATCH] = np.sum(e * e), npts, npts
    if kind == "zeros":
        return np.zeros((3, NACC_PAD), dtype=T)
    return split_blocks(rng, tot, 3, T)


def rotation(rng, angle=None):
    ax = rng.normal(size=3)
    ax *= (rng.uniform(0, np.pi) if angle is None else angle) / np.linalg.norm(ax)
    return so3_exp(ax)


def random_pose(rng, T, trans=3.0):
    return rT(np.concatenate([rotation(rng).ravel(), rng.normal(size=3) * trans]), T)
