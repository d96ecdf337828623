"""Reference, noise, error model, kernel-order emulation and comparator for the fused Gumbel-softmax correspondence
(csrc/kernels_soft_svd.h: gumbel_fwd_kernel, gumbel_bwd_q_kernel, gumbel_bwd_t_kernel).

A plain module (no fixtures): the tests put this directory on sys.path and import it.  tests/test_gumbel_ref.py proves the model and the
comparator on a CPU against `emulate`, tests/test_gpu_gumbel.py holds the kernels to them on the GPU.

THE REFERENCE (`reference`) is a float64 torch restatement of nn.py:43-70 on inputs already rounded to the dtype under test:
    s = |x - y[:3]|^2,  g = -log(-log(u + eps) + eps),  l = (g - s) / tau,  p = softmax_j l,  out = p @ y
with eps and 1 / tau rounded the way the host rounds them ((T)eps, (T)(1.0 / tau)); gradients are autograd of <cot, out>.  It is pinned to
oracle.dicp_oracle.nn_gumbel in float64.

THE NOISE.  `hash_uniform(seed, N, n, m)` restates mix32 and the key chain of gumbel_fwd_kernel in numpy:
    key = mix32(mix32(seed ^ cloud 0x9E3779B9) ^ i 0x85EBCA6B),  u = (mix32(key ^ (j 0xC2B2AE35 + 0x27D4EB2F)) >> 8) 2^-24
The values are 24-bit integers times 2^-24: exact in float32 and float64, so the restated U can be injected bit for bit.

THE BOUND (`bounds`) is a first-order forward error model with safety factor 1, written out in closed form (the sensitivities of a softmax
are known: d out_k / d l_j = p_j (y_jk - out_k)).  u_T is the unit roundoff (2^-24 / 2^-53), ulp = 2 u_T.  Per rounded intermediate:
    add, subtract, multiply                 0.5 ulp
    float32 on the device                   v_exp_f32, v_rcp_f32, v_log_f32 1 ulp each (csrc/dicp_math.h); __logf = v_log_f32 times ln 2 in
                                            extended precision, rounded once more: 1.5 ulp; __expf(x) = v_exp_f32(fl(x fl(log2 e))): the
                                            argument carries 1 ulp, so the result 1 ulp + 2 |x| u_T, as point_math_ref.py treats m_tanh
    float64 on the device, the reference    log, exp 1 ulp (the documented bound of the device library's and of the C library's); '/' 0.5 ulp
The chain, pair by pair (absolute errors d.):
    d_a = x_a - y_a (u_T), d_a^2 (3 u_T), s = (d_0^2 + d_1^2) + d_2^2          ds  = 5 u_T s
    a0 = u + eps: the nearest number to u + eps, and u itself is one             da0 = min(u_T a0, eps)
    L1 = log a0                                                                  dL1 = da0 / a0 + c_log |L1|
    a1 = -L1 + eps                                                               da1 = dL1 + u_T a1
    g = -log a1                                                                  dg  = da1 / a1 + c_log |g|
    t = g - s,  l = t (1 / tau)                                                  dl  = (dg + ds + u_T |t|) / tau + u_T |l|
The online softmax.  Term j enters as e_j = exp(l_j - M_j) (M_j the running maximum including j) and is rescaled by exp(M - M') at each of
the R_j later steps that raise the maximum; sc = exp(0) = 1 is exact, as is a product with it.  The same e_j and sc enter S and acc, so their
relative errors
    eps_j = u_T (2 + c_x |l_j - M_j|) + u_T (2 R_j + c_x (M_final - M_j))        c_x = 3 (float32: the subtraction and the argument), 1 (float64)
reach out_k with the sensitivity p_j |y_jk - out_k|, like dl_j.  What S and acc do NOT share -- the product e y, the products with sc, and
the sequential sums (a partial sum rounds once per step: u_T times the sum of the partial sums, at most m u_T sum |term|, which is the
form used for the reference's own sums, whose order is torch's) -- reaches out_k as
    u_T [ W(p |y_k|) + sum_j p_j |y_jk| (1 + R_j) + |out_k| (W(p) + sum_j p_j R_j) ],   W(t) = sum_j (t_1 + .. + t_j)
i.e. the share of the sums is m u_T (sum p |y| + |out|) in the worst case, not sum p |y - out|.  1 / S (1 ulp float32, 0.5 ulp float64) and
the product with it close the forward.  lse = M + log S carries sum_j p_j (dl_j + eps_j) + the sums' share + c_log |log S| + u_T |lse|.
The backward recomputes l_j (dl_j again), p_j = exp(l_j - lse) (relative pi_j = dl_j + d lse + the exp's u_T (2 + c_x |l_j - lse|)),
gy_j = sum_k go_k y_jk and D = sum_k go_k out_k ((C + 1) u_T of the absolute terms; D also d out from the forward), dl_j = p_j (gy_j - D),
the three products into g[.] (dl, the difference, the product, the sequential sum over m) and the final scale -2 / tau; the target pass
the same per query, with two sums per step over n.  No cancellation is assumed in the backward: a gradient is bounded by the sum of its
terms' bounds.

THE REFERENCE'S OWN ERROR.  The reference is float64 arithmetic: the bound adds the same model evaluated with float64 constants and the
order-free form of the sums.  For float32 under test that is parts in 1e9 of the bound.

FLOOR is 2^-126 (float32) / 2^-1022 (float64), as in point_math_ref.py: a result of that size may be flushed, and v_exp_f32 flushes
denormal results (a far target whose e underflows), so every pair adds FLOOR times its sensitivity.

THE EMULATION (`emulate`) runs the three kernels' operation order in numpy in the dtype under test: sequential j, the running maximum, the
exp(M - Mn) rescale, tiles of GUM_TILE (which only matter to the injected faults), and the two backward passes.  It exists so that model
and comparator are proved on a CPU; `fault=` switches on one of the deliberately wrong variants the comparator must refuse.
"""
import numpy as np
import torch

from oracle import dicp_oracle as O

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
U_T = {F32: 2.0 ** -24, F64: 2.0 ** -53}
FLOOR = {F32: 2.0 ** -126, F64: 2.0 ** -1022}
BLOCK, GUM_TILE = 256, 512
MASK = np.uint64(0xFFFFFFFF)
# the float32 forms the constants describe (held to the source by tests/test_gumbel_ref.py::test_model_matches_the_sources)
DEVICE_FORMS = {"log_t": "__logf(v)", "exp_t": "__expf(v)", "tile": "constexpr int GUM_TILE = 512;"}
NOISE_EDGES = (0.0, 2.0 ** -24, 2.0 ** -23, 0.5, 1 - 2.0 ** -22, 1 - 2.0 ** -23, 1 - 2.0 ** -24)


def np_dtype(dtype):
    if isinstance(dtype, torch.dtype):
        return np.dtype({torch.float32: np.float32, torch.float64: np.float64}[dtype])
    return np.dtype(dtype)


def round_to(a, dtype):
    """values -> float64 numpy array of values representable in dtype"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.astype(np_dtype(dtype)).astype(np.float64)


def par(v, dtype):
    """a scalar parameter of the call in the kernel's type: (T)v"""
    return float(np_dtype(dtype).type(v))


# ---------------------------------------------------------------- the noise
def mix32(v):
    v = np.asarray(v, dtype=np.uint64) & MASK
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x7feb352d)) & MASK
    v = v ^ (v >> np.uint64(15))
    v = (v * np.uint64(0x846ca68b)) & MASK
    return v ^ (v >> np.uint64(16))


def hash_uniform(seed, N, n, m, cloud_term=True):
    """(N,n,m) float64: the draw gumbel_uniform makes for (seed, cloud, i, j).  cloud_term=False is a deliberately wrong key (a test's negative control)."""
    cloud, i, j = (np.arange(k, dtype=np.uint64) for k in (N, n, m))
    kc = mix32(np.uint64(int(seed) & 0xFFFFFFFF) ^ ((cloud * np.uint64(0x9E3779B9)) & MASK if cloud_term else np.zeros(N, dtype=np.uint64)))
    key = mix32(kc[:, None] ^ ((i * np.uint64(0x85EBCA6B)) & MASK)[None, :])
    h = mix32(key[:, :, None] ^ ((j * np.uint64(0xC2B2AE35) + np.uint64(0x27D4EB2F)) & MASK)[None, None, :])
    return (h >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


# ---------------------------------------------------------------- the reference
def reference(x, y, U, eps, tau, dtype, cot=None):
    """x (N,n,3), y (N,m,c), U (N,n,m), cot (N,n,c): float64 values representable in dtype -> dict of float64 numpy arrays: out, and with cot gx, gy"""
    e, it = par(eps, dtype), par(1.0 / tau, dtype)
    xt = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=cot is not None)
    yt = torch.tensor(np.asarray(y, dtype=np.float64), requires_grad=cot is not None)
    ut = torch.tensor(np.asarray(U, dtype=np.float64))
    d = xt[:, :, None, :3] - yt[:, None, :, :3]
    s = (d * d).sum(-1)
    g = -torch.log(-torch.log(ut + e) + e)
    l = (g - s) * it
    p = torch.softmax(l, dim=2)
    out = p @ yt
    res = {"out": out.detach().numpy(), "p": p.detach().numpy(), "l": l.detach().numpy(), "g": g.detach().numpy(), "s": s.detach().numpy()}
    if cot is not None:
        (out * torch.tensor(np.asarray(cot, dtype=np.float64))).sum().backward()
        res["gx"], res["gy"] = xt.grad.numpy(), yt.grad.numpy()
    return res


def oracle_out(x, y, U, eps, tau):
    return O.nn_gumbel(torch.tensor(x), torch.tensor(y), eps, tau, U=torch.tensor(U)).numpy()


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


def _W(t, ar, axis):
    """the rounding share of a sum of the non-negative terms t along axis, per unit of u_T"""
    if ar.sequential:
        return np.cumsum(t, axis=axis).sum(axis=axis)
    return t.shape[axis] * t.sum(axis=axis)


def _model(ar, x, y, U, e, it, ref, cot):
    u = ar.u
    c = y.shape[2]
    p, l, g, s = ref["p"], ref["l"], ref["g"], ref["s"]
    out = ref["out"]
    ds = 5 * u * s
    a0 = U + e
    da0 = np.minimum(u * a0, e)
    L1 = np.log(a0)
    dL1 = da0 / a0 + ar.c_log * np.abs(L1)
    a1 = -L1 + e
    da1 = dL1 + u * a1
    dg = da1 / a1 + ar.c_log * np.abs(g)
    dl = it * (dg + ds + u * np.abs(g - s)) + u * np.abs(l)
    Mfin = l.max(axis=2, keepdims=True)
    if ar.sequential:
        Mrun = np.maximum.accumulate(l, axis=2)
        rise = np.zeros_like(l)
        rise[:, :, 1:] = Mrun[:, :, 1:] > Mrun[:, :, :-1]
        R = rise.sum(axis=2, keepdims=True) - np.cumsum(rise, axis=2)           # rescales after j
    else:
        Mrun, R = np.broadcast_to(Mfin, l.shape), np.zeros_like(l)
    eps_j = ar.c_e0 + ar.c_ex * np.abs(l - Mrun) + 2 * u * R + ar.c_ex * (Mfin - Mrun)
    ay = np.abs(y)[:, None, :, :]                                                # (N,1,m,c)
    dev = np.abs(y[:, None, :, :] - out[:, :, None, :])                          # (N,n,m,c)
    pe = p * (dl + eps_j)
    WS = _W(p, ar, 2)                                                            # (N,n)
    pR = (p * R).sum(2)
    b_out = np.empty_like(out)
    for k in range(c):
        t = p * ay[..., k]
        b_out[..., k] = ((pe * dev[..., k]).sum(2) + u * (_W(t, ar, 2) + (t * (1 + R)).sum(2) + np.abs(out[..., k]) * (WS + pR))
                         + (ar.c_rcp + u) * np.abs(out[..., k]) + ar.floor * (1 + dev[..., k].sum(2)))
    res = {"out": b_out}
    if cot is None:
        return res
    logS = np.log(np.exp(l - Mfin).sum(2))
    L = Mfin[..., 0] + logS
    dL = pe.sum(2) + u * (WS + pR) + ar.c_log * np.abs(logS) + u * np.abs(L)
    pi = dl + dL[..., None] + ar.c_e0 + ar.c_ex * np.abs(l - L[..., None])
    go = cot
    gyd = np.einsum("bik,bjk->bij", go, y)
    dgyd = (c + 1) * u * np.einsum("bik,bjk->bij", np.abs(go), np.abs(y))
    D = (go * out).sum(-1)
    dD = (np.abs(go) * b_out).sum(-1) + (c + 1) * u * np.abs(go * out).sum(-1)
    w = gyd - D[..., None]
    dlj = p * w
    ddl = np.abs(dlj) * (pi + 2 * u) + p * (dgyd + dD[..., None])
    d3 = np.abs(x[:, :, None, :3] - y[:, None, :, :3])                           # (N,n,m,3)
    b_gx = np.empty(x.shape)
    for a in range(3):
        t = np.abs(dlj) * d3[..., a]
        tot = (ddl * d3[..., a]).sum(2) + 2 * u * t.sum(2) + u * _W(t, ar, 2)
        b_gx[..., a] = 2 * it * tot + 2 * u * 2 * it * t.sum(2) + ar.floor * (1 + 2 * it * (np.abs(w) * d3[..., a]).sum(2))
    b_gy = np.empty(y.shape)
    for k in range(c):
        t1 = p * np.abs(go[..., k])[:, :, None]
        tot = (t1 * (pi + u)).sum(1)
        t = t1
        fl = np.abs(go[..., k])[:, :, None] * np.ones_like(p)
        if k < 3:
            t2 = 2 * it * np.abs(dlj) * d3[..., k]
            tot = tot + (2 * it * ddl * d3[..., k] + 4 * u * t2).sum(1)
            t = t1 + t2
            fl = fl + 2 * it * np.abs(w) * d3[..., k]
        b_gy[..., k] = tot + 2 * u * _W(t, ar, 1) + ar.floor * (1 + fl.sum(1))
    res["gx"], res["gy"] = b_gx, b_gy
    return res


def bounds(x, y, U, eps, tau, dtype, cot=None, ref=None):
    """the model's bound on |kernel - reference| for out (and gx, gy): the dtype's own error plus the float64 reference's"""
    e, it = par(eps, dtype), par(1.0 / tau, dtype)
    x, y, U = (np.asarray(t, dtype=np.float64) for t in (x, y, U))
    ref = ref if ref is not None else reference(x, y, U, eps, tau, dtype, cot)
    cot = None if cot is None else np.asarray(cot, dtype=np.float64)
    with np.errstate(all="ignore"):
        own = _model(Arith(dtype, True), x, y, U, e, it, ref, cot)
        theirs = _model(Arith(F64, False), x, y, U, e, it, ref, cot)
    return {k: own[k] + theirs[k] for k in own}


def compare(got, want, bound):
    """-> (ok, worst |got - want| / bound, its index).  Non-finite values must agree as such."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    if not np.array_equal(fin, np.isfinite(got)) or not np.isfinite(bound[fin]).all():
        return False, np.inf, None
    ratio = np.zeros(want.shape)
    err = np.abs(got - want)[fin]
    ratio[fin] = np.where(err > 0, err / np.maximum(bound[fin], 1e-300), 0.0)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else None
    worst = float(ratio.max()) if ratio.size else 0.0
    return worst <= 1.0, worst, at


def hold(got, x, y, U, eps, tau, dtype, cot=None):
    """compare a result dict (out[, gx, gy]) with the reference under the model's bound -> {name: (ok, worst ratio, index)}"""
    x, y, U = (np.asarray(t, dtype=np.float64) for t in (x, y, U))
    ref = reference(x, y, U, eps, tau, dtype, cot)
    b = bounds(x, y, U, eps, tau, dtype, cot, ref)
    return {k: compare(got[k], ref[k], b[k]) for k in b if k in got}


# ---------------------------------------------------------------- the kernels' operation order
def emulate(x, y, U, eps, tau, dtype, cot=None, fault=None, at=None):
    """The three kernels in numpy in `dtype`.  fault: None | "no_rescale_at_tile_start" | "skip_tile_last" | "bwd_noise_shift" | "off_16u"
    (1 / S of query `at` = (cloud, i) off by 16 u_T).  -> out, lse[, gx, gy]"""
    T = np_dtype(dtype).type
    x, y, U = (np.asarray(t).astype(T) for t in (x, y, U))
    e, it = T(eps), T(1.0 / tau)
    N, n, _ = x.shape
    m, c = y.shape[1], y.shape[2]
    if T is np.float32:
        log2e = np.float32(1.4426950408889634)
        exp_t = lambda v: np.exp2((v * log2e).astype(T))
    else:
        exp_t = np.exp
    log_t = np.log

    def logit(xi, yj, uu):
        d0, d1, d2 = xi[..., 0] - yj[..., 0], xi[..., 1] - yj[..., 1], xi[..., 2] - yj[..., 2]
        g = -log_t(-log_t(uu + e) + e)
        return (g - (d0 * d0 + d1 * d1 + d2 * d2)) * it

    with np.errstate(all="ignore"):
        M = np.full((N, n), -np.inf, dtype=T)
        S = np.zeros((N, n), dtype=T)
        acc = np.zeros((N, n, c), dtype=T)
        for j in range(m):
            if fault == "skip_tile_last" and j % GUM_TILE == GUM_TILE - 1:
                continue
            yj = y[:, j, :][:, None, :]
            l = logit(x, yj, U[:, :, j])
            Mn = np.where(l > M, l, M)
            sc, ee = exp_t(M - Mn), exp_t(l - Mn)
            if fault == "no_rescale_at_tile_start" and j > 0 and j % GUM_TILE == 0:
                sc = np.where(l > M, T(1), sc)
            S = S * sc + ee
            acc = acc * sc[..., None] + ee[..., None] * yj
            M = Mn
        invS = T(1) / S
        if fault == "off_16u":
            invS[at] = invS[at] * T(1 + 16 * U_T[np_dtype(dtype)])
        out = acc * invS[..., None]
        lse = M + log_t(S)
        res = {"out": out, "lse": lse}
        if cot is None:
            return res
        go = np.asarray(cot).astype(T)
        Ub = np.roll(U, -1, axis=2) if fault == "bwd_noise_shift" else U
        D = np.zeros((N, n), dtype=T)
        for k in range(c):
            D = D + go[..., k] * out[..., k]
        gq = np.zeros((N, n, 3), dtype=T)
        for j in range(m):
            yj = y[:, j, :][:, None, :]
            p = exp_t(logit(x, yj, Ub[:, :, j]) - lse)
            gyd = np.zeros((N, n), dtype=T)
            for k in range(c):
                gyd = gyd + go[..., k] * yj[..., k]
            dl = p * (gyd - D)
            for a in range(3):
                gq[..., a] = gq[..., a] + dl * (x[..., a] - yj[..., a])
        res["gx"] = (-T(2) * it) * gq
        gt = np.zeros((N, m, c), dtype=T)
        for i in range(n):
            r = x[:, i, :][:, None, :]
            gi = go[:, i, :][:, None, :]
            p = exp_t(logit(r, y, Ub[:, i, :]) - lse[:, i][:, None])
            gd = np.zeros((N, m), dtype=T)
            for k in range(c):
                gd = gd + gi[..., k] * y[..., k]
                gt[..., k] = gt[..., k] + p * gi[..., k]
            dl = p * (gd - D[:, i][:, None]) * (T(2) * it)
            for a in range(3):
                gt[..., a] = gt[..., a] + dl * (r[..., a] - y[..., a])
        res["gy"] = gt
    return res


# ---------------------------------------------------------------- inputs
CHOSEN = (0, 63, 64, 255)          # lanes of block 0; the last live lane of the tail block joins them


def random_set(N, n, m, c, dtype, seed, offset=0.0):
    """clouds in [0,3) + offset, columns 3:6 unit normals, U uniform, a cotangent: float64 arrays of values representable in dtype"""
    r = np.random.default_rng(seed)
    x = r.uniform(0, 3, (N, n, 3)) + offset
    y = r.uniform(0, 3, (N, m, c))
    y[..., :3] += offset
    if c == 6:
        y[..., 3:] = r.normal(size=(N, m, 3))
        y[..., 3:] /= np.linalg.norm(y[..., 3:], axis=-1, keepdims=True)
    U = r.integers(0, 2 ** 24, (N, n, m)).astype(np.float64) * 2.0 ** -24
    cot = r.normal(size=(N, n, c))
    return tuple(round_to(t, dtype) for t in (x, y, U, cot))


def _base(N, n, m, c, dtype, seed):
    """queries in [0,1)^3, targets in [8,9)^3 (every pair at least 7 apart per axis), noise in [0.2, 0.8] (g within [-0.5, 1.5]: it cannot
    overturn a gap of 2 in distance)"""
    r = np.random.default_rng(seed)
    x = r.uniform(0, 1, (N, n, 3))
    y = r.uniform(8, 9, (N, m, c))
    if c == 6:
        y[..., 3:] = r.normal(size=(N, m, 3))
        y[..., 3:] /= np.linalg.norm(y[..., 3:], axis=-1, keepdims=True)
    U = np.floor(r.uniform(0.2, 0.8, (N, n, m)) * 2 ** 24) * 2.0 ** -24
    cot = r.normal(size=(N, n, c))
    return x, y, U, cot


def chosen_queries(n):
    return sorted(set(q for q in CHOSEN + (n - 1,) if q < n))


def designed_sets(dtype, N=3, n=300, m=1100, c=3):
    """name -> (x, y, U, cot, eps, tau): the inputs of section 2 of tests/test_gpu_gumbel.py, all at tau = 0.05 unless named otherwise.
    Every set is also an input of the CPU tests (the emulation stays inside the bound, the faults leave it)."""
    sets = {}
    Q = chosen_queries(n)
    tau = 0.05
    for J in sorted(set(j for j in (0, 511, 512, 513, 1023, 1024, m - 1) if j < m)):
        # one target within 1e-3 of the chosen queries, everything else at least 2 away
        x, y, U, cot = _base(N, n, m, c, dtype, 100 + J)
        for q in Q:
            x[:, q] = np.array([5.0, 5.0, 5.0]) + 1e-4 * (q % 7)
        y[:, J, :3] = np.array([5.0, 5.0, 5.0]) + 5e-4
        sets["near_j%d" % J] = (x, y, U, cot, 1e-20, tau)
    for name, sign in (("ascending", -1.0), ("descending", 1.0)):
        # logits strictly monotone in j: one line of targets, the queries beside its start, constant noise
        x, y, U, cot = _base(N, n, m, c, dtype, 200)
        rj = np.linspace(1.0, 3.0, m) if sign > 0 else np.linspace(3.0, 1.0, m)
        y[..., 0], y[..., 1], y[..., 2] = rj[None, :], 0.0, 0.0
        x[..., 0] = 0.0
        x[..., 1:] = (x[..., 1:] - 0.5) * 0.02
        U[:] = 0.5
        sets[name] = (x, y, U, cot, 1e-20, tau)
    if m > 512:
        # the maximum first appears at j = 512 (a tile's first element), over a first tile that carries weight before it
        x, y, U, cot = _base(N, n, m, c, dtype, 300)
        x[..., :] = (x - 0.5) * 0.02
        y[..., 0], y[..., 1], y[..., 2] = np.linspace(2.0, 3.0, m)[None, :], 0.0, 0.0
        y[:, 512, 0] = 0.5
        U[:] = 0.5
        sets["max_at_512"] = (x, y, U, cot, 1e-20, tau)
        # two equal maxima in different tiles
        x, y, U, cot = _base(N, n, m, c, dtype, 400)
        for q in Q:
            x[:, q] = np.array([5.0, 5.0, 5.0]) + 1e-4 * (q % 7)
        j1, j2 = 100, min(700, m - 1)
        y[:, j1, :3] = y[:, j2, :3] = np.array([5.0, 5.0, 5.0]) + 5e-4
        if c == 6:
            y[:, j2, 3:] = -y[:, j1, 3:]
        U[:, :, j2] = U[:, :, j1]
        sets["equal_maxima"] = (x, y, U, cot, 1e-20, tau)
    if m >= 16 and n >= 14:
        # noise edges: query e duels over two targets whose logits are within 0.4 of each other -- one carries the edge draw, the other u = 0.5 --
        # so the value of g(u) decides the split ("dominant"); query 7 + e carries the edge on a pair 2 away ("background")
        for eps in (1e-10, 1e-20):
            ed = par(eps, dtype)
            gum = lambda v: -np.log(-np.log(v + ed) + ed)
            x, y, U, cot = _base(N, n, m, c, dtype, 500)
            x[..., 0] += 40.0                                                   # everything not placed below is far from every target
            for b in range(N):
                j0 = (0, min(505, m - 16), m - 16)[b % 3]
                for k, ue in enumerate(NOISE_EDGES):
                    je, jc = j0 + 2 * k, j0 + 2 * k + 1
                    here = np.array([20.0 * k, 20.0, 20.0])
                    x[b, k], x[b, 7 + k] = here, here + np.array([0.0, 6.0, 0.0])
                    gap = gum(ue) - gum(0.5)
                    se, sc = (gap, 0.0) if gap > 0 else (0.0, -gap)
                    y[b, je, :3] = here + np.array([np.sqrt(se + 0.02), 0.0, 0.0])
                    y[b, jc, :3] = here - np.array([np.sqrt(sc), 0.0, 0.0])
                    U[b, k, je], U[b, k, jc] = ue, 0.5
                    U[b, 7 + k, je] = ue                                        # background: (6^2 + ..) away, whatever it draws
            sets["noise_edges_eps%g" % eps] = (x, y, U, cot, eps, tau)
    return {k: tuple(round_to(t, dtype) for t in v[:4]) + v[4:] for k, v in sets.items()}
