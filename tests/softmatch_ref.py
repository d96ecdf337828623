"""Reference, error model, kernel-order emulation and comparator for soft_match_features (dicp_amd/match.py; csrc/softmatch.hip, the rules:
csrc/dicp_softmatch.h), for ONE cloud.

A plain module (no fixtures), on the model of tests/gumbel_ref.py: the tests put this directory on sys.path and import it.
tests/test_softmatch_host.py proves model and comparator on a CPU against `emulate` and the g++ build of the header,
tests/test_gpu_softmatch.py holds the kernels to them on the GPU.

THE REFERENCE (`reference`).  The scores come from match_ref.scores -- the exact fma chain in the dtype under test, so the logits' inputs
are bit-identical to the kernel's -- and the candidates are the finite scores of the rows below the counts.  Everything after that is
float64 torch: c = (T)(-2.0 / tau) as a float64 number, l = c s, p = softmax over the candidates, out = p @ values, idx = the first
candidate in (score, index) order, prob = p at idx.  Gradients are autograd of <cot, out> with the scores and the values as leaves; the
score's own derivative (ds_ij / dx_i = -y_j, ds_ij / dy_j = y_j - x_i) carries the leaf's gradient to the tables in float64.

THE BOUND (`bounds`) is a first-order forward error model with safety factor 1 in gumbel_ref.py's closed form and with its per-operation
constants (add, subtract, multiply, fma 0.5 ulp; float32 on the device: v_exp_f32, v_rcp_f32 1 ulp, __logf 1.5 ulp, __expf's argument
scaled once more; float64 and the reference: exp, log 1 ulp, '/' 0.5 ulp; u_T the unit roundoff).  The chain:
    l = c s                                                                       dl  = u_T |l|
The online softmax in blocks (`schedule`: the rows a state meets, block by block, and the states that are joined at the end).  Term j
enters as e_j = exp(l_j - M_j), M_j the running maximum after its block's, and is rescaled by exp(M - M') at each of the R_j later raises
(a join that lifts the state counts as one).  |l_j - M_j| and the sum of the raises after it add up to M_final - l_j whatever the order, so
    eps_j = c_e0 + c_ex (M_final - l_j) + 2 u_T R_j
reaches out_k with the sensitivity p_j |v_jk - out_k|, like dl_j.  What S and the sums do not share -- the products e v, the products with
the rescale factors, the sequential sums (u_T times the sum of the partial sums W, per state, plus the join) -- reaches out_k as
    u_T [ W(p |v_k|) + sum_j p_j |v_jk| (1 + R_j) + |out_k| (W(p) + sum_j p_j R_j) ]
and 1 / S and the product with it close the forward.  lse = M + log S carries sum_j p_j (dl_j + eps_j) + the sums' share + c_log |log S| +
u_T |lse|; prob = exp(l_best - lse) the relative error dl + d lse + c_e0 + c_ex |l_best - lse|.
The backward recomputes l_j (dl_j again) and p_j = exp(l_j - lse): relative pi_j = dl_j + d lse + c_e0 + c_ex |l_j - lse|;
gv_ij = g_i . v_j and delta_i = g_i . out_i ((C + 1) u_T of the absolute terms, delta also d out from the forward); a_ij = p_ij (gv_ij -
delta_i); then with NO cancellation assumed -- a gradient is bounded by the sum of its terms' bounds --
    gfx_ic = -c sum_j a_ij y_jc,   gfy_jc = c (y_jc sum_i a_ij - sum_i a_ij x_ic),   gvalues_jk = sum_i p_ij g_ik
each with its products, its sequential sum and the final scale.  The bound adds the same model with float64 constants and order-free sums
for the reference's own error, and FLOOR (2^-126 / 2^-1022) per term for results that may be flushed.

THE EMULATION (`emulate`) runs the kernels' operation order in numpy in the dtype under test; `fault=` switches on one of the deliberately
wrong variants the comparator must refuse.
"""
import numpy as np
import torch

import match_ref as mr

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
U_T = {F32: 2.0 ** -24, F64: 2.0 ** -53}
FLOOR = {F32: 2.0 ** -126, F64: 2.0 ** -1022}
SOFT_ROWS = 16                      # csrc/dicp_softmatch.h
SM_STAGE_TILES, SM_STAGE_WORDS = 8, 256     # csrc/softmatch.hip
FAULTS = ("no_rescale", "skip_tile_edge", "pad_row", "gfy_sign", "lse_no_max", "off_16u")


def np_dtype(dtype):
    if isinstance(dtype, torch.dtype):
        return np.dtype({torch.float32: np.float32, torch.float64: np.float64}[dtype])
    return np.dtype(dtype)


def scale(tau, dtype):
    """c of the definition as a float64 number"""
    return float(np_dtype(dtype).type(-2.0 / float(tau)))


def stage_rows(D):
    """rows of fy per LDS stage of the matrix-core form"""
    Dp = 2 * ((D + 1) // 2)
    return 32 * max(1, min(SM_STAGE_TILES, SM_STAGE_WORDS // Dp))


def schedule(form, m):
    """the states of one query and the blocks of rows each meets, in order: [[block, ...], ...]; state 0 takes the others at the end"""
    if form == "mfma":
        j = np.arange(m)
        halves = []
        for kh in (0, 1):
            mine = j[((j % 32) // 4) % 2 == kh]
            halves.append([mine[(mine // 32) == t] for t in range((m + 31) // 32)])
        return [[b for b in h if b.size] for h in halves]
    return [[np.arange(b, min(b + SOFT_ROWS, m)) for b in range(0, m, SOFT_ROWS)]]


# ---------------------------------------------------------------- the reference
def candidates(fx, fy, x_rows=None, y_rows=None):
    """-> s (n, m) in the tables' dtype (NaN outside the counts), cand (n, m) bool"""
    n, m = fx.shape[0], fy.shape[0]
    xr = n if x_rows is None else int(x_rows)
    yr = m if y_rows is None else int(y_rows)
    s = np.full((n, m), np.nan, dtype=fx.dtype)
    if xr and yr:
        s[:xr, :yr] = mr.scores(np.ascontiguousarray(fx[:xr]), np.ascontiguousarray(fy[:yr]))
    return s, np.isfinite(s)


def reference(fx, fy, values, tau, x_rows=None, y_rows=None, cot=None):
    """fx (n, D), fy (m, D), values (m, C) numpy arrays of the dtype under test -> dict of float64 arrays: out, idx (int64), prob, p, l, cand
    and with cot (n, C): gfx, gfy, gvalues"""
    dt = fx.dtype
    s, cand = candidates(fx, fy, x_rows, y_rows)
    c = scale(tau, dt)
    n, m = s.shape
    yr = m if y_rows is None else int(y_rows)
    s64 = np.where(cand, s.astype(np.float64), 0.0)
    st = torch.tensor(s64, requires_grad=cot is not None)
    v64 = np.zeros(values.shape, dtype=np.float64)
    v64[:yr] = values[:yr].astype(np.float64)                   # pad rows' values are never read
    vt = torch.tensor(v64, requires_grad=cot is not None)
    ct = torch.tensor(cand)
    l = torch.where(ct, c * st, torch.full_like(st, -np.inf))
    some = ct.any(dim=1)
    lmax = torch.where(some, l.max(dim=1).values, torch.zeros(n, dtype=torch.float64))
    e = torch.where(ct, torch.exp(l - lmax[:, None]), torch.zeros_like(st))
    S = e.sum(dim=1)
    p = e / torch.where(some, S, torch.ones_like(S))[:, None]
    out = p @ vt
    key = np.where(cand, s64, np.inf)
    idx = np.where(cand.any(axis=1), np.argmin(key, axis=1), -1).astype(np.int64)        # (argmin: the first of equal scores)
    pn = p.detach().numpy()
    res = {"out": out.detach().numpy(), "idx": idx, "p": pn, "l": np.where(cand, c * s64, -np.inf), "cand": cand, "c": c,
           "prob": np.where(idx >= 0, pn[np.arange(n), np.clip(idx, 0, None)], 0.0),
           "lse": np.where(cand.any(axis=1), (lmax + torch.log(torch.where(some, S, torch.ones_like(S)))).detach().numpy(), np.inf)}
    if cot is not None:
        g = np.where(cand.any(axis=1)[:, None], np.asarray(cot, dtype=np.float64), 0.0)      # a dead query's cotangent may hold anything
        (out * torch.tensor(g)).sum().backward()
        gs = st.grad.numpy() * cand                             # = c a_ij
        x64, y64 = fx.astype(np.float64), fy.astype(np.float64)
        x64, y64 = np.where(cand.any(axis=1)[:, None], x64, 0.0), np.where(cand.any(axis=0)[:, None], y64, 0.0)   # (rows that take no part may hold anything)
        res["gfx"] = -gs @ y64
        res["gfy"] = gs.sum(axis=0)[:, None] * y64 - gs.T @ x64
        res["gvalues"] = vt.grad.numpy()
        res["a"] = gs / c
    return res


# ---------------------------------------------------------------- the bound
class Arith:
    def __init__(self, dtype, sequential=True):
        self.dt = np_dtype(dtype)
        self.u, self.floor = U_T[self.dt], FLOOR[self.dt]
        fast = self.dt == F32
        self.c_log = (3.0 if fast else 2.0) * self.u        # __logf 1.5 ulp; log 1 ulp
        self.c_e0 = 2.0 * self.u                            # v_exp_f32 / exp: 1 ulp
        self.c_ex = (3.0 if fast else 1.0) * self.u         # per unit of |argument|: its subtraction (+ fl(x fl(log2 e)))
        self.c_rcp = (2.0 if fast else 1.0) * self.u        # v_rcp_f32 1 ulp; '/' 0.5 ulp
        self.sequential = sequential


def _W(t, ar, axis, streams=None):
    """the rounding share of a sum of the non-negative terms t along axis, per unit of u_T: the partial sums after every step that adds
    something (adding an exact zero rounds nothing); streams: the index arrays of the partial sums that are joined at the end"""
    if not ar.sequential:
        return t.shape[axis] * t.sum(axis=axis)
    if streams is None:
        return (np.cumsum(t, axis=axis) * (t > 0)).sum(axis=axis)
    tot = t.sum(axis=axis) * (len(streams) - 1)             # the joins
    for st in streams:
        ts = np.take(t, st, axis=axis)
        tot = tot + (np.cumsum(ts, axis=axis) * (ts > 0)).sum(axis=axis)
    return tot


def _raises(l, sched):
    """R (n, m): the rescales a term meets after it enters, in float64 on the reference's logits (-inf: no candidate)"""
    n, m = l.shape
    R = np.zeros((n, m))
    Mfin = l.max(axis=1)
    for blocks in sched:
        if not blocks:
            continue
        Mb = np.stack([l[:, b].max(axis=1) for b in blocks], axis=1)            # (n, B)
        Mrun = np.maximum.accumulate(Mb, axis=1)
        rise = np.zeros_like(Mb)
        rise[:, 1:] = Mrun[:, 1:] > Mrun[:, :-1]
        after = rise.sum(axis=1, keepdims=True) - np.cumsum(rise, axis=1) + (Mrun[:, -1:] < Mfin[:, None])
        for k, b in enumerate(blocks):
            R[:, b] = after[:, k:k + 1]
    return R


def _model(ar, fx, fy, values, ref, cot, sched):
    u = ar.u
    cand, p, c = ref["cand"], ref["p"], abs(ref["c"])
    some = cand.any(axis=1)
    l = np.where(cand, ref["l"], 0.0)
    out = ref["out"]
    n, m = p.shape
    C = values.shape[1]
    v = np.where(cand.any(axis=0)[:, None], values.astype(np.float64), 0.0)
    Mfin = np.where(some, np.where(cand, l, -np.inf).max(axis=1, initial=-np.inf), 0.0)
    R = _raises(np.where(cand, l, -np.inf), sched) * cand if ar.sequential else np.zeros((n, m))
    streams = [np.concatenate(b) for b in sched if b] if ar.sequential else None
    dl = u * np.abs(l)
    eps = (ar.c_e0 + ar.c_ex * (Mfin[:, None] - l) + 2 * u * R) * cand
    pe = p * (dl + eps)
    WS = _W(p, ar, 1, streams)
    pR = (p * R).sum(axis=1)
    av = np.abs(v)
    b_out = np.zeros_like(out)
    for k in range(C):
        dev = np.abs(v[None, :, k] - out[:, k, None]) * cand
        t = p * av[None, :, k]
        b_out[:, k] = ((pe * dev).sum(axis=1) + u * (_W(t, ar, 1, streams) + (t * (1 + R)).sum(axis=1) + np.abs(out[:, k]) * (WS + pR))
                       + (ar.c_rcp + u) * np.abs(out[:, k]) + ar.floor * (1 + dev.sum(axis=1))) * some
    S = np.where(cand, np.exp(l - Mfin[:, None]), 0.0).sum(axis=1)
    logS = np.log(np.where(some, S, 1.0))
    L = Mfin + logS
    dL = pe.sum(axis=1) + u * (WS + pR) + ar.c_log * np.abs(logS) + u * np.abs(L)
    pi = (dl + dL[:, None] + ar.c_e0 + ar.c_ex * np.abs(l - L[:, None])) * cand
    rows = np.arange(n)
    best = np.clip(ref["idx"], 0, None)
    res = {"out": b_out, "prob": (ref["prob"] * (pi[rows, best] + u) + ar.floor) * some}
    if cot is None:
        return res
    g = np.where(some[:, None], np.asarray(cot, dtype=np.float64), 0.0)
    x = np.where(some[:, None], fx.astype(np.float64), 0.0)
    y = np.where(cand.any(axis=0)[:, None], fy.astype(np.float64), 0.0)
    gv = g @ v.T
    dgv = (C + 1) * u * (np.abs(g) @ av.T)
    delta = (g * out).sum(axis=1)
    ddelta = (np.abs(g) * b_out).sum(axis=1) + (C + 1) * u * np.abs(g * out).sum(axis=1)
    w = (gv - delta[:, None]) * cand
    a = p * w
    da = np.abs(a) * (pi + 2 * u) + p * (dgv + ddelta[:, None]) * cand
    aa, aw = np.abs(a), np.abs(w)
    D = fx.shape[1]
    b_gx, b_gy = np.zeros((n, D)), np.zeros((m, D))
    sa_abs, dsa = aa.sum(axis=0), da.sum(axis=0) + u * _W(aa, ar, 0)
    for ch in range(D):
        t = aa * np.abs(y[None, :, ch])
        tot = (da * np.abs(y[None, :, ch])).sum(axis=1) + u * t.sum(axis=1) + u * _W(t, ar, 1)
        b_gx[:, ch] = c * tot + 2 * u * c * t.sum(axis=1) + ar.floor * (1 + c * (aw * np.abs(y[None, :, ch])).sum(axis=1))
        t = aa * np.abs(x[:, ch, None])
        dA = (da * np.abs(x[:, ch, None])).sum(axis=0) + u * t.sum(axis=0) + u * _W(t, ar, 0)
        mag = np.abs(y[:, ch]) * sa_abs + t.sum(axis=0)
        b_gy[:, ch] = c * (np.abs(y[:, ch]) * dsa + dA + u * mag) + 2 * u * c * mag + ar.floor * (1 + c * (aw * (np.abs(y[None, :, ch]) + np.abs(x[:, ch, None]))).sum(axis=0))
    b_gv = np.zeros((m, C))
    for k in range(C):
        t = p * np.abs(g[:, k, None])
        b_gv[:, k] = (t * (pi + u)).sum(axis=0) + u * _W(t, ar, 0) + ar.floor * (1 + (np.abs(g[:, k, None]) * cand).sum(axis=0))
    res["gfx"], res["gfy"], res["gvalues"] = b_gx * some[:, None], b_gy, b_gv
    return res


def bounds(fx, fy, values, tau, ref, cot=None, form="valu"):
    """the model's bound on |kernel - reference| per output: the dtype's own error in the form's order plus the float64 reference's"""
    sched = schedule(form, fy.shape[0])
    with np.errstate(all="ignore"):
        own = _model(Arith(fx.dtype, True), fx, fy, values, ref, cot, sched)
        theirs = _model(Arith(F64, False), fx, fy, values, ref, cot, sched)
    return {k: own[k] + theirs[k] for k in own}


def compare(got, want, bound):
    """-> (ok, worst |got - want| / bound, its index).  Non-finite values must agree as such; a zero bound asks for equality."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False, np.inf, None
    fin = np.isfinite(want)
    if not np.array_equal(fin, np.isfinite(got)) or not np.isfinite(bound[fin]).all():
        return False, np.inf, None
    ratio = np.zeros(want.shape)
    err = np.abs(got - want)[fin]
    ratio[fin] = np.where(err > 0, err / np.maximum(bound[fin], 1e-300), 0.0)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else None
    worst = float(ratio.max()) if ratio.size else 0.0
    return worst <= 1.0, worst, at


def hold(got, fx, fy, values, tau, x_rows=None, y_rows=None, cot=None, form="valu"):
    """compare a result dict (out, idx, prob[, gfx, gfy, gvalues]) with the reference under the model's bound
    -> {name: (ok, worst ratio, index)}; idx must be equal"""
    ref = reference(fx, fy, values, tau, x_rows, y_rows, cot)
    b = bounds(fx, fy, values, tau, ref, cot, form)
    res = {k: compare(got[k], ref[k], b[k]) for k in b if k in got}
    if "idx" in got:
        same = bool(np.array_equal(np.asarray(got["idx"]), ref["idx"]))
        res["idx"] = (same, 0.0 if same else np.inf, None)
    return res


# ---------------------------------------------------------------- the kernels' operation order
def emulate(fx, fy, values, tau, x_rows=None, y_rows=None, cot=None, form="valu", fault=None, at=0):
    """The kernels in numpy in the tables' dtype, the forward in `form`'s order -> out, idx, prob, lse[, gfx, gfy, gvalues].
    fault: one of FAULTS ("off_16u": 1 / S of query `at` off by 16 u_T)."""
    T = fx.dtype.type
    n, D = fx.shape
    m, C = fy.shape[0], values.shape[1]
    xr = n if x_rows is None else int(x_rows)
    yr = m if y_rows is None else int(y_rows)
    s, cand = candidates(fx, fy, x_rows, y_rows if fault != "pad_row" else None)
    if fault == "pad_row":
        cand[xr:] = False
    c = T(-2.0 / float(tau))
    if T is np.float32:
        log2e = np.float32(1.4426950408889634)
        exp_t = lambda a: np.exp2((a * log2e).astype(T))
    else:
        exp_t = np.exp
    ninf = T(-np.inf)
    with np.errstate(all="ignore"):
        l = (c * s).astype(T)
        states = []
        for blocks in schedule(form, m):
            M, S, acc = np.full(n, ninf, dtype=T), np.zeros(n, dtype=T), np.zeros((n, C), dtype=T)
            bs, bj = np.full(n, np.inf, dtype=T), np.full(n, -1, dtype=np.int64)
            for bi, b in enumerate(blocks):
                if fault == "skip_tile_edge":
                    b = b[b % SOFT_ROWS != SOFT_ROWS - 1] if bi == 0 else b
                if not b.size:
                    continue
                lb = np.where(cand[:, b], l[:, b], ninf)
                Mb = lb.max(axis=1)
                up = Mb > M
                sc = np.where(up, exp_t(M - np.where(up, Mb, M)), T(1))
                if fault == "no_rescale":
                    sc = np.ones(n, dtype=T)
                S, acc = (S * sc).astype(T), (acc * sc[:, None]).astype(T)
                M = np.where(up, Mb, M)
                for j in b:
                    on = cand[:, j]
                    e = np.where(on, exp_t(np.where(on, l[:, j] - M, T(0))), T(0)).astype(T)
                    S = np.where(on, S + e, S).astype(T)
                    for k in range(C):
                        acc[:, k] = np.where(on, mr.fma(e, np.full(n, values[j, k], dtype=T), acc[:, k], T), acc[:, k])
                    better = on & ((s[:, j] < bs) | ((s[:, j] == bs) & (j < bj)))
                    bs, bj = np.where(better, s[:, j], bs), np.where(better, j, bj)
            states.append((M, S, acc, bs, bj))
        M, S, acc, bs, bj = states[0]
        for (M2, S2, acc2, bs2, bj2) in states[1:]:
            has = bj2 >= 0
            up = has & (M2 > M)
            sc = np.where(up, exp_t(M - np.where(up, M2, M)), T(1))
            S, acc = (S * sc).astype(T), (acc * sc[:, None]).astype(T)
            M = np.where(up, M2, M)
            f = np.where(has, exp_t(np.where(has, M2 - M, T(0))), T(0)).astype(T)
            S = np.where(has, mr.fma(S2, f, S, T), S)
            for k in range(C):
                acc[:, k] = np.where(has, mr.fma(acc2[:, k], f, acc[:, k], T), acc[:, k])
            better = has & ((bs2 < bs) | ((bs2 == bs) & (bj2 < bj)))
            bs, bj = np.where(better, bs2, bs), np.where(better, bj2, bj)
        some = bj >= 0
        inv = (T(1) / np.where(some, S, T(1))).astype(T)
        if fault == "off_16u":
            inv[at] = inv[at] * T(1 + 16 * U_T[np.dtype(T)])
        out = np.where(some[:, None], (acc * inv[:, None]).astype(T), T(0))
        lse = np.where(some, (M + np.log(np.where(some, S, T(1))).astype(T)).astype(T), T(np.inf))
        prob = np.where(some, exp_t(np.where(some, (c * bs).astype(T) - lse, T(0))), T(0)).astype(T)
        res = {"out": out, "idx": bj, "prob": prob, "lse": lse}
        if cot is None:
            return res
        g = np.asarray(cot).astype(T)
        Lb = lse if fault != "lse_no_max" else np.where(some, np.log(np.where(some, S, T(1))).astype(T), T(np.inf))
        delta = np.zeros(n, dtype=T)
        for k in range(C):
            delta = mr.fma(g[:, k], out[:, k], delta, T)
        live = some[:, None] & cand
        gvd = np.zeros((n, m), dtype=T)
        for k in range(C):
            gvd = mr.fma(g[:, k, None], np.where(cand.any(axis=0), values[:, k], T(0))[None, :], gvd, T)
        p = np.where(live, exp_t(np.where(live, l - Lb[:, None], T(0))), T(0)).astype(T)
        a = np.where(live, (p * (gvd - delta[:, None]).astype(T)).astype(T), T(0))
        G = np.zeros((n, D), dtype=T)
        for j in range(m):
            on = live[:, j]
            if on.any():
                G = np.where(on[:, None], mr.fma(a[:, j, None], np.broadcast_to(fy[j][None, :], (n, D)), G, T), G)
        res["gfx"] = np.where(some[:, None], ((-c) * G).astype(T), T(0))
        sa, A, GV = np.zeros(m, dtype=T), np.zeros((m, D), dtype=T), np.zeros((m, C), dtype=T)
        for i in range(n):
            on = live[i]
            if not on.any():
                continue
            sa = np.where(on, (sa + a[i]).astype(T), sa)
            A = np.where(on[:, None], mr.fma(a[i][:, None], np.broadcast_to(fx[i][None, :], (m, D)), A, T), A)
            GV = np.where(on[:, None], mr.fma(p[i][:, None], np.broadcast_to(g[i][None, :], (m, C)), GV, T), GV)
        ysafe = np.where((np.arange(m) < yr)[:, None] & np.isfinite(fy), fy, T(0))
        gfy = (c * mr.fma(ysafe, np.broadcast_to(sa[:, None], (m, D)), -A, T)).astype(T)
        if fault == "gfy_sign":
            gfy = -gfy
        rowlive = (np.arange(m) < yr)[:, None]
        res["gfy"] = np.where(rowlive, gfy, T(0))
        res["gvalues"] = np.where(rowlive, GV, T(0))
    return res


# ---------------------------------------------------------------- inputs
def random_case(n, m, D, C, dtype, seed, spread=1.0):
    """unit-scale descriptors with every query near one row of fy (so that small temperatures keep weight on more than one row), values
    in [-1, 1), a normal cotangent -> fx, fy, values, cot in dtype"""
    r = np.random.default_rng(seed)
    fy = r.standard_normal((m, D)) / np.sqrt(D)
    fx = fy[r.integers(0, m, n)] + spread * 0.2 * r.standard_normal((n, D)) / np.sqrt(D)
    values = r.uniform(-1, 1, (m, C))
    cot = r.standard_normal((n, C))
    return tuple(np.ascontiguousarray(t.astype(np_dtype(dtype))) for t in (fx, fy, values, cot))
