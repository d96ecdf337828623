"""Reference, error model and comparator for the per-point arithmetic of one ICP iteration (csrc/dicp_math.h: point_weights, point_forward,
point_backward) and for the stand-alone loss weight (csrc/kernels_soft_svd.h: loss_eval, loss_weight{,_bwd}_kernel).

A plain module (no fixtures): the tests put this directory on sys.path and import it.  tests/test_point_math_ref.py holds the g++ build of the
header to it on a CPU, tests/test_gpu_point_math.py the kernels on the GPU.

THE REFERENCE is a float64 torch restatement of the reference semantics, given the matches (ICP.py:137-201, loss.py:21-58): q = C p,
e3 = q + r - y, the trim gate on |e3|, the robust loss on |e3| (pt2pt) or |n . e3| (pt2pl), w = w_init tw lw, u = (sqrt(w + 1e-10) - 1e-5)^2,
J = [q^ | -I] or [(q^)^T n | -n], A = sum u J^T J, b = sum u J^T e, cost = sum u e^2.  `semantic_forward` writes exactly that with the oracle's
loss_weight and skew; `Chain` writes the same values operation by operation so that every rounded intermediate can be perturbed, and the tests
pin the two to each other.  Gradients are torch autograd of <G_A, A> + <g_b, b>; the norms use e/|e| with 0 at e == 0, and the hard Huber
weight is torch.where(en > metric, metric / en, 1), whose gradient at en == 0 is 0 * -inf = NaN (kept on purpose).  Inputs are first rounded
to the dtype under test; the call's parameters are rounded the way wp_val rounds them ((float)double).

THE BOUND is a first-order forward error model with safety factor 1.  Every rounded intermediate t_k of the chain is written
t_k (1 + d_k) + a_k with d_k = a_k = 0, so that autograd gives do/dd_k = do/dt_k t_k and do/da_k = do/dt_k for every output o; the points are
independent, so one .sum().backward() per output gives all points at once.  With ulp = 2 u_T (u_T the unit roundoff 2^-24 / 2^-53: a correctly
rounded operation is 0.5 ulp = u_T relative)

    B(o) = ulp * sum_k c_k |do/dd_k|  +  FLOOR * (1 + sum_k |do/da_k|)

The intermediates: the products and partial sums of q, q + r, e3, the squares and partial sums of d3^2, d3, the products and sums of e, the
tanh argument (three operations), th, tw, the loss quotient and its operands, lw, w_init alive, w_init tw, w, w + 1e-10, root, ws, u, and
every product and difference that enters a slot.  c_k, from the project (csrc/dicp_math.h:60-68), not from any output:
    add, subtract, multiply                     0.5 ulp
    float32 on the device: v_sqrt_f32, v_rcp_f32, v_exp_f32   1 ulp each, so m_div = a * rcp(b) is 1.5 ulp and m_sqrt 1 ulp
    float64, and the g++ build of the header:   sqrt and '/' 0.5 ulp; tanh / tanhf 2 ulp (the documented bound of the C library's and of
                                                the device library's tanh)
    the stand-alone loss kernels use plain '/' in every build: 0.5 ulp
m_tanh on the device is th = 1 - 2 rcp(E + 1), E = exp2(a), a = fl(x c), c = fl(2 log2 e).  Its absolute error from its three operations:
a carries 0.5 ulp (the constant) + 0.5 ulp (the product), so E carries 1 ulp (v_exp_f32) + |a| ln 2 = 2 |x| ulp (the argument);
s = E + 1 carries E / (E + 1) of that + 0.5 ulp; R = rcp(s) one more ulp; 2 R is exact and 1 - 2 R rounds once more.  With 2 R = 1 - th and
E / (E + 1) = (1 + th) / 2:

    |dth| <= ulp * [ (1 - th) ((1 + th) / 2 * (1 + 2 |x|) + 1.5) + 0.5 |th| ]        (2 ulp = 2.4e-7 at x = 0; 0.5 ulp at th = +1; 3.5 at -1)

th enters the model with that ABSOLUTE error (a node t + h A, c = 1).  The adjoint forms 1 - th th from that rounded th: the model's tanh
node differentiates the same way, and the product th th is one more rounded intermediate (0.5 ulp of 1, under a difference of 1e-4).  A sum over n points gets the sum of its terms' bounds plus
n u_T sum |term| for the summation (an atomic sum of in-degree D: D u_T sum |term|).

The backward.  The kernels do not differentiate the forward operation by operation; they run the closed-form adjoint.  The model gives every
intermediate's ADJOINT a relative error of its own (a hook on its gradient, g (1 + e_k), e_k = 0) and adds ulp * sum_k cb_k |dg/de_k| to the
forward terms (which reach a gradient through the second derivative).  cb_k = c_k + 0.5: the adjoint takes the operation's local derivative
(at most the operation again) and is accumulated once.  The slots' own adjoints -- where the cotangents Gs, gb enter -- get the roundings the
closed form spends on one monomial Gs_ab j_a j_b before it reaches u-bar: pt2pl 13 (Gj: a product and 5 sums; j . Gj: a product and 6 sums;
+ e jgb), pt2pt 17 (a cross product 2, - Gs 1, the product with Q 1, a trace of 12 terms, + e . Jgb): 6.5 / 8.5 ulp.  Because the hook sits on
every product that enters a slot, a gradient is bounded by the sum of its monomials' magnitudes, not by its own (cancelling) value.

THE REFERENCE'S OWN ERROR.  The reference runs in float64, so for float64 under test it is no more exact than the code under test (a build that
contracts a * b + c into one rounding, as the device does, differs from it by as much as it differs from the truth).  Every term of B therefore
carries, with the same sensitivity, the reference's own rounding as well: 2^-52 times 0.5 per operation (torch's float64 operations are correctly
rounded), 2 |th| for its tanh, 1 per adjoint.  For float32 under test that adds parts in 1e9 of the bound.

FLOOR is 2^-126 (float32) / 2^-1022 (float64): a result of that size may be flushed or lose its last bits, whatever produced it, and
v_sqrt_f32 / v_rcp_f32 / v_exp_f32 flush denormal arguments and results (dicp_math.h:65).  Beyond first order -- an intermediate of the
reference above the dtype's largest number, below half its smallest denormal, or (device float32) a denormal argument of sqrt / rcp -- the
reference is evaluated with that intermediate replaced by what the format makes of it (+-inf, 0), the point is marked `extreme`, and its
w and slots are held to: the same class (finite or not: whether 0 * inf comes out as an infinity or as NaN hangs on values below FLOOR), and
the bound on the finite ones with the sensitivities that are themselves finite.  The GRADIENTS of an extreme point are held to the plain float64 evaluation (1e40 and
1e-60 fit a double) or to the one with the format's replacement, wholly to one of them, and at two documented edges to NaN (extreme_gradients;
the stand-alone loss: loss_extreme).  No other slack.

TIES.  The hard decisions d3 < trim_dist, en > metric, en < metric, w > match_thresh are taken on computed values.  A point is a tie when its
reference value lies within 8 ulp of the threshold plus the model's own bound on that value (the decision variable carries the error of the
chain before it: 8 ulp of trim_dist is far less than the rounding of q + r - y for a cloud 25 km from the origin).  A tie is not held to the
bound; its outputs must equal, wholly, the reference with the decision taken one way or the other.  Random inputs contain no tie (asserted on
the reference alone; the seeds are chosen so); only the edge sets place some.
"""
import ctypes
import math
import os

import numpy as np
import torch

from oracle import dicp_oracle as O

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
U = {F32: 2.0 ** -24, F64: 2.0 ** -53}
FLOOR = {F32: 2.0 ** -126, F64: 2.0 ** -1022}
FMAX = {F32: float(np.finfo(np.float32).max), F64: float(np.finfo(np.float64).max)}
DENORM_MIN = {F32: 2.0 ** -149, F64: 2.0 ** -1074}
TIE_ULPS = 8.0
REF_ULP = 2.0 ** -52           # the reference is evaluated in float64: its own intermediates round too
REF_TANH_ULPS = 2.0            # torch's float64 tanh
REF_ADJOINT = 1.0              # an adjoint of the reference's autograd: one product, one accumulation
GPU_POINTS = 2048         # clouds of one point per configuration in tests/test_gpu_point_math.py (its inputs are checked for ties on the CPU)
NACC = 30
ACC_B, ACC_COST, ACC_SUMW, ACC_NMATCH = 21, 27, 28, 29
LOSS_CODE = {"none": 0, "huber": 1, "cauchy": 2, "trim": 3}
# the device float32 forms the constants describe (held to the source by tests/test_point_math_ref.py::test_model_matches_the_sources)
DEVICE_FORMS = {
    "m_sqrt": "__builtin_amdgcn_sqrtf(x)",
    "m_div": "a * __builtin_amdgcn_rcpf(b)",
    "m_tanh": ("__builtin_amdgcn_exp2f(x * 2.8853900817779268f)", "1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f)"),
}


def np_dtype(dtype):
    if isinstance(dtype, torch.dtype):
        return np.dtype({torch.float32: np.float32, torch.float64: np.float64}[dtype])
    return np.dtype(dtype)


class Arith:
    """The constants of one build: dtype x {"device", "host"}"""

    def __init__(self, dtype, build):
        assert build in ("device", "host")
        self.dt = np_dtype(dtype)
        self.build = build
        self.u, self.ulp, self.floor, self.fmax, self.dmin = U[self.dt], 2 * U[self.dt], FLOOR[self.dt], FMAX[self.dt], DENORM_MIN[self.dt]
        self.fast = self.dt == F32 and build == "device"          # the one-instruction forms
        self.c_sqrt = 1.0 if self.fast else 0.5
        self.c_div = 1.5 if self.fast else 0.5
        self.c_libm_tanh = 2.0

    def par(self, v):
        """a parameter of the call in the kernel's scalar type (wp_val)"""
        return float(np.float32(v)) if self.dt == F32 else float(v)

    def tanh_abs_ulps(self, x, th):
        if self.fast:
            return (1 - th) * ((1 + th) / 2 * (1 + 2 * x.abs().clamp(max=1000.0)) + 1.5) + 0.5 * th.abs()      # (beyond |x| = 1000, 1 + th or 1 - th is 0: no 0 * inf)
        return self.c_libm_tanh * th.abs()


def round_to(a, dtype):
    """numpy / torch values -> float64 torch tensor of values representable in dtype"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return torch.tensor(a.astype(np_dtype(dtype)).astype(np.float64))


# ---------------------------------------------------------------- the tape of rounded intermediates
class Tape:
    def __init__(self, ar, ieee=False, plain=False):
        self.ar = ar
        self.plain = plain              # flag the intermediates that leave the dtype's range, but keep their float64 values (1e40 and 1e-60 fit a double)
        self.ieee = ieee                # an overflowed intermediate is +-inf (values only); otherwise the largest number (a graph autograd can still walk)
        self.nodes = []                 # (name, d, a, e, c, cb)
        self.perturb = {}               # name -> (point, relative error): a deliberately wrong intermediate, for the tests of the comparator
        self.extreme = None             # (n,) bool: an intermediate left the dtype's range
        self.values = {}

    def _flag(self, bad):
        bad = bad.reshape(bad.shape[0], -1).any(1)
        self.extreme = bad if self.extreme is None else (self.extreme | bad)

    def fit(self, x):
        """what the format makes of a value outside its range"""
        ar = self.ar
        xd = x.detach()
        over = xd.abs() > ar.fmax
        under = (xd != 0) & (xd.abs() < ar.dmin / 2)
        if bool(over.any()) or bool(under.any()):
            self._flag(over | under)
            if self.plain:
                return x
            x = torch.where(over, torch.sign(xd) * (math.inf if self.ieee else ar.fmax), x)
            x = torch.where(under, torch.zeros_like(xd), x)
        return x

    def flush_arg(self, x):
        """the argument of v_sqrt_f32 / v_rcp_f32: a denormal is read as 0 (device float32 only)"""
        if not self.ar.fast:
            return x
        xd = x.detach()
        den = (xd != 0) & (xd.abs() < self.ar.floor)
        if bool(den.any()):
            self._flag(den)
            if self.plain:
                return x
            x = torch.where(den, torch.zeros_like(xd), x)
        return x

    def r(self, x, name, c=0.5, cb=None, mask=None, tanh=False):
        """one rounded intermediate: x (1 + d) + a, its adjoint g (1 + e).  tanh: the node is tanh(x) with an absolute error (tanh(x) + d A + a)"""
        x = self.fit(x)
        cref = 0.5 if c > 0 else 0.0        # the float64 reference's own rounding of this intermediate (correctly rounded operations)
        d = torch.zeros_like(x, requires_grad=True)
        a = torch.zeros_like(x, requires_grad=True)
        e = torch.zeros_like(x, requires_grad=True)
        if tanh:
            xd = x.detach()
            dsq = torch.zeros_like(x, requires_grad=True)
            A = self.ar.tanh_abs_ulps(xd, torch.tanh(xd))
            y = _TanhSeen.apply(x, d * A + a, dsq)
            self.nodes.append((name + ".sq", dsq, torch.zeros_like(x, requires_grad=True), torch.zeros_like(x, requires_grad=True), 0.5, 0.0, 0.5))
            cref = torch.where(A > 0, REF_TANH_ULPS * torch.tanh(xd).abs() / torch.where(A > 0, A, torch.ones_like(A)), torch.zeros_like(A))
        elif mask is not None:
            y = x * (1 + d * mask) + a * mask
        else:
            y = x * (1 + d) + a
        if name in self.perturb:
            bump = torch.zeros(x.shape[0], dtype=torch.float64)
            bump[self.perturb[name][0]] = self.perturb[name][1]
            y = y * (1 + bump.reshape((-1,) + (1,) * (x.dim() - 1)))
        if y.requires_grad:
            y.register_hook(lambda g, e=e: g * (1 + e))
        self.nodes.append((name, d, a, e, c, c + 0.5 if cb is None else cb, cref))
        self.values[name] = y
        return y


class _SqrtZ(torch.autograd.Function):
    """sqrt whose gradient is g * (0 at x == 0), as torch's norm: e/|e| with 0 at e == 0 -- and a NaN that arrives still leaves as NaN (NaN * 0)"""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.sqrt(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        pos = x > 0
        return g * torch.where(pos, 0.5 / torch.sqrt(torch.where(pos, x, torch.ones_like(x))), torch.zeros_like(x))


def safe_sqrt(x):
    return _SqrtZ.apply(x)


def _sum3(T, t, name):
    s = T.r(t[..., 0] + t[..., 1], name + ".s1")
    return T.r(s + t[..., 2], name + ".s2")


def _dot3(T, a, b, name):
    return _sum3(T, T.r(a * b, name + ".p"), name)


def _cross3(T, a, b, name):
    i1, i2 = [1, 2, 0], [2, 0, 1]
    return T.r(T.r(a[..., i1] * b[..., i2], name + ".p1") - T.r(a[..., i2] * b[..., i1], name + ".p2"), name)


class _TanhSeen(torch.autograd.Function):
    """th = tanh(x) + pert whose derivative is 1 - th^2 of the PERTURBED th: the adjoint (dicp_math.h: 1 - s.th * s.th) is formed from the rounded th, so
    near saturation the error of th reaches the gate's gradient through the cancellation in 1 - th^2, not only through tw"""

    @staticmethod
    def forward(ctx, x, pert, dsq):
        th = torch.tanh(x) + pert
        ctx.save_for_backward(th, dsq)
        return th

    @staticmethod
    def backward(ctx, g):
        th, dsq = ctx.saved_tensors
        return g * (1 - th * th * (1 + dsq)), g, None         # dsq: the rounding of th * th, an absolute 0.5 ulp of 1 under the difference


def _soft_gate(T, ar, k, thr, x, name):
    """0.5 tanh(k (thr - x) - 3) + 0.5, loss.py:54"""
    arg = T.r(T.r(k * T.r(thr - x, name + ".diff"), name + ".kx") - 3.0, name + ".arg")
    th = T.r(arg, name + ".th", c=1.0, tanh=True)
    return T.r(0.5 * th + 0.5, name + ".tw"), th


def _decide(dec, flips, name, value, thr, cond):
    dec[name] = (value, thr)
    if flips is not None and name in flips:
        cond = cond ^ flips[name]
    return cond


def tri(i, j):
    return i * 6 - (i * (i - 1)) // 2 + (j - i)


class Chain:
    """One iteration's per-point chain for n independent points, each with its own pose.
    cfg: mode "pt2pt" | "pt2pl", loss "none" | "huber" | "cauchy" | "trim", diff, trim_on, trim_dist, tanh_k, metric, match_thresh
    inp: p, y, nrm (n,3), C (n,3,3), r (n,3), w_init (n,), alive (n,): float64 tensors of values representable in the dtype under test
    flips: {decision: (n,) bool} takes a hard decision the other way on those points"""

    def __init__(self, ar, cfg, inp, flips=None, grads=False, safe=True, ieee=False, perturb=None, plain=False):
        """safe: the branch torch.where does not take is evaluated where it is finite (for the sensitivities); not safe: as the reference writes it
        (its gradient at en == 0 is NaN).  ieee: see Tape"""
        self.ar, self.cfg = ar, cfg
        T = self.T = Tape(ar, ieee, plain)
        T.perturb = perturb or {}
        self.dec = {}
        pl = cfg["mode"] == "pt2pl"
        leaf = lambda t: t.clone().requires_grad_(grads)
        self.p, self.y, self.nrm, self.C, self.rr, self.w_init = (leaf(inp[k]) for k in ("p", "y", "nrm", "C", "r", "w_init"))
        alive = inp["alive"]
        n = self.p.shape[0]
        one, zero = torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        k, tau, dl, thr = ar.par(cfg["tanh_k"]), ar.par(cfg["trim_dist"]), ar.par(cfg["metric"]), ar.par(cfg["match_thresh"])
        q = _sum3(T, T.r(self.C * self.p[:, None, :], "q.p"), "q")                              # ICP.py:137
        e3 = T.r(T.r(q + self.rr, "qr") - self.y, "e3")                                          # ICP.py:144,148
        d3sq = _sum3(T, T.r(e3 * e3, "d3sq.p"), "d3sq")
        d3 = T.r(safe_sqrt(T.flush_arg(d3sq)), "d3", c=ar.c_sqrt)
        if pl:
            e = _dot3(T, e3, self.nrm, "e")                                                      # ICP.py:146
            en = e.abs()
        else:
            e, en = None, d3
        tw = one
        if cfg["trim_on"]:
            if cfg["diff"]:
                tw, _ = _soft_gate(T, ar, k, tau, d3, "trim")
            else:
                tw = _decide(self.dec, flips, "d3<trim", d3, tau, d3.detach() < tau).to(torch.float64)      # loss.py:58
        lw = one
        if cfg["loss"] == "huber":
            if cfg["diff"]:                                                                      # loss.py:30
                dl2 = T.r(torch.full((n,), dl * dl, dtype=torch.float64), "dl2")                # (the product of the rounded parameter with itself is one more rounding)
                lw = T.r(dl2 / T.flush_arg(T.r(dl2 + T.r(en * en, "en2"), "hub.den")), "lw", c=ar.c_div)
            else:                                                                                # loss.py:32
                cond = _decide(self.dec, flips, "en>metric", en, dl, en.detach() > dl)
                lw = T.r(torch.where(cond, dl / (torch.where(cond, en, one) if safe else en), one), "lw", c=ar.c_div, mask=cond.to(torch.float64))
        elif cfg["loss"] == "cauchy":                                                            # loss.py:41
            t = T.r(en / dl, "cau.t", c=ar.c_div)
            lw = T.r(1.0 / T.flush_arg(T.r(1.0 + T.r(t * t, "cau.t2"), "cau.den")), "lw", c=ar.c_div)
        elif cfg["loss"] == "trim":
            if cfg["diff"]:
                lw, _ = _soft_gate(T, ar, k, dl, en, "ltrim")
            else:
                lw = _decide(self.dec, flips, "en<metric", en, dl, en.detach() < dl).to(torch.float64)
        w0 = T.r(self.w_init * alive, "w0")
        w = T.r(T.r(w0 * tw, "w0tw") * lw, "w")                                                  # ICP.py:169
        c10, c5 = (float(np.float32(1e-10)), float(np.float32(1e-5))) if ar.dt == F32 else (1e-10, 1e-5)
        root = T.r(safe_sqrt(T.flush_arg(T.r(w + c10, "w+"))), "root", c=ar.c_sqrt)              # ICP.py:194
        ws = T.r(root - c5, "ws")
        u = T.r(ws * ws, "u")
        cbs = 6.5 if pl else 8.5
        S = torch.zeros(n, NACC, dtype=torch.float64)
        col = lambda v: v[:, None]
        if pl:
            j = torch.cat((_cross3(T, self.nrm, q, "nxq"), -self.nrm), 1)                        # ICP.py:175-176
            uj = T.r(col(u) * j, "uj")
            ia = [a for a in range(6) for b in range(a, 6)]
            ib = [b for a in range(6) for b in range(a, 6)]
            S = self._put(S, [tri(a, b) for a, b in zip(ia, ib)], T.r(uj[:, ia] * j[:, ib], "A", cb=cbs))
            S = self._put(S, list(range(ACC_B, ACC_B + 6)), T.r(uj * col(e), "b", cb=cbs))
            S = self._put(S, [ACC_COST], col(T.r(T.r(u * e, "ue") * e, "cost")))
        else:                                                                                    # ICP.py:178-183: J = [q^, -I]
            qq = _dot3(T, q, q, "qq")
            S = self._put(S, [tri(a, a) for a in range(3)], T.r(col(u) * T.r(col(qq) - T.r(q * q, "q.q"), "qq-"), "A.diag", cb=cbs))
            S = self._put(S, [tri(0, 1), tri(0, 2), tri(1, 2)], T.r(col(u) * T.r(-q[:, [0, 0, 1]] * q[:, [1, 2, 2]], "q.off"), "A.off", cb=cbs))
            S = self._put(S, [tri(3, 3), tri(4, 4), tri(5, 5)], T.r(col(u) * torch.ones(n, 3, dtype=torch.float64), "A.rr", c=0.0, cb=cbs))
            sk = ((0, 4, -1, 2), (0, 5, 1, 1), (1, 3, 1, 2), (1, 5, -1, 0), (2, 3, -1, 1), (2, 4, 1, 0))      # (row, column, sign, element of q): q^ in the C-r block
            sg = torch.tensor([float(x[2]) for x in sk], dtype=torch.float64)
            S = self._put(S, [tri(x[0], x[1]) for x in sk], T.r(col(u) * (sg * q[:, [x[3] for x in sk]]), "A.skew", cb=cbs))
            exq = _cross3(T, e3, q, "exq")
            S = self._put(S, [ACC_B, ACC_B + 1, ACC_B + 2], T.r(col(u) * exq, "b.C", cb=cbs))
            S = self._put(S, [ACC_B + 3, ACC_B + 4, ACC_B + 5], -T.r(col(u) * e3, "b.r", cb=cbs))
            S = self._put(S, [ACC_COST], col(T.r(u * _dot3(T, e3, e3, "ee"), "cost")))
        rows = 1.0 if pl else 3.0
        S = self._put(S, [ACC_SUMW], col(T.r(rows * w, "sumw")))
        S = self._put(S, [ACC_NMATCH], col(rows * _decide(self.dec, flips, "w>thresh", w, thr, w.detach() > thr).to(torch.float64)))
        self.w, self.slots = w, S
        self.extreme = T.extreme if T.extreme is not None else torch.zeros(n, dtype=torch.bool)
        self.n = n

    @staticmethod
    def _put(S, cols, vals):
        return S.index_add(1, torch.tensor(cols), vals)

    # ------------------------------------------------------------ outputs and their bounds
    def forward_outputs(self):
        """(n,31): w, then the 30 slots"""
        return torch.cat((self.w[:, None], self.slots), 1)

    def backward_outputs(self, Gs, gb):
        """Gs (n,36) symmetric (= G_A + G_A^T), gb (n,6) -> (n,22): d/dp 3, d/dy 3, d/dnormal 3, d/dw_init 1, d/dC 9, d/dr 3 of <G_A, A> + <g_b, b>"""
        coef = torch.zeros(self.n, NACC, dtype=torch.float64)
        for a in range(6):
            for b in range(a, 6):
                coef[:, tri(a, b)] = Gs[:, a * 6 + b] * (0.5 if a == b else 1.0)
        coef[:, ACC_B:ACC_B + 6] = gb
        L = (coef * self.slots).sum()
        g = torch.autograd.grad(L, [self.p, self.y, self.nrm, self.w_init, self.C, self.rr], create_graph=True, allow_unused=True)
        g = [torch.zeros_like(x) if gi is None else gi for gi, x in zip(g, [self.p, self.y, self.nrm, self.w_init, self.C, self.rr])]
        return torch.cat((g[0], g[1], g[2], g[3][:, None], g[4].reshape(self.n, 9), g[5]), 1)

    def bound(self, out, backward=False):
        return tape_bound(self.T, out, backward, self.extreme)

    def decision_bounds(self):
        """{decision: (value, threshold, tie (n,) bool)}: within TIE_ULPS ulp of the threshold plus the model's bound on the value"""
        res = {}
        for name, (value, thr) in self.dec.items():
            B = tape_bound(self.T, value[:, None], False, self.extreme)[:, 0] if value.requires_grad else torch.zeros(self.n, dtype=torch.float64)
            v = value.detach()
            res[name] = (v, thr, (v - thr).abs() <= TIE_ULPS * self.ar.ulp * abs(thr) + B)
        return res


def tape_bound(T, out, backward, extreme):
    """out (n,K) -> B (n,K) float64 (detached).  The K outputs' sensitivities come from one batched reverse pass.  Every term carries the error of
    the dtype under test and, with the same sensitivity, the reference's own (REF_ULP: it is float64 too)."""
    ar = T.ar
    n, K = out.shape
    B = torch.full((n, K), ar.floor, dtype=torch.float64)
    if not out.requires_grad:
        return B
    leaves = []
    for nd in T.nodes:
        leaves += [nd[1], nd[2]] + ([nd[3]] if backward else [])
    per = 3 if backward else 2
    sel = torch.zeros(K, n, K, dtype=torch.float64)
    for k in range(K):
        sel[k, :, k] = 1.0
    gs = torch.autograd.grad(out, leaves, grad_outputs=sel, retain_graph=True, allow_unused=True, is_grads_batched=True)
    ext = extreme[None, :, None] if extreme is not None else None
    for i, (_, d, a, e, c, cb, cref) in enumerate(T.nodes):
        for g, f in zip(gs[per * i:per * i + per], (ar.ulp * c + REF_ULP * cref, ar.floor, ar.ulp * cb + REF_ULP * REF_ADJOINT)):
            if g is None:
                continue
            t = g.detach().abs()
            if isinstance(f, torch.Tensor):
                t = t * f.reshape((1,) + tuple(f.shape))
                f = 1.0
            elif f == 0.0:
                continue
            t = t.reshape(K, n, -1)
            if ext is not None:
                t = torch.where(ext & ~torch.isfinite(t), torch.zeros_like(t), t)
            B += f * t.sum(2).transpose(0, 1)
    return B


def semantic_forward(cfg, inp, ar):
    """The same outputs straight from the reference's tensor expressions (ICP.py:137-201) with the oracle's loss_weight and skew: (n,31)"""
    p, y, nrm, C, r = inp["p"], inp["y"], inp["nrm"], inp["C"], inp["r"]
    n = p.shape[0]
    q = (C @ p[:, :, None])[:, :, 0]
    e3 = q + r - y
    k, tau, dl, thr = ar.par(cfg["tanh_k"]), ar.par(cfg["trim_dist"]), ar.par(cfg["metric"]), ar.par(cfg["match_thresh"])
    pl = cfg["mode"] == "pt2pl"
    err = (e3 * nrm).sum(1, keepdim=True) if pl else e3
    # ((1, n, r) inputs: the 3-D form, one weight per row for every loss)
    tw = O.loss_weight(e3[None], "trim", tau, cfg["diff"], k)[0] if cfg["trim_on"] else torch.ones(n, dtype=torch.float64)
    lw = O.loss_weight(err[None], cfg["loss"], dl, cfg["diff"], k)[0] if cfg["loss"] != "none" else torch.ones(n, dtype=torch.float64)
    w = inp["w_init"] * inp["alive"] * tw * lw
    c10, c5 = (float(np.float32(1e-10)), float(np.float32(1e-5))) if ar.dt == F32 else (1e-10, 1e-5)
    u = (torch.sqrt(w + c10) - c5) ** 2
    sk = O.skew(q[None])[0]                                                                      # (n,3,3)
    if pl:
        J = torch.cat(((sk.transpose(1, 2) @ nrm[:, :, None])[:, :, 0], -nrm), 1)[:, None, :]   # (n,1,6)
        ev = err[:, :, None]
    else:
        J = torch.cat((sk, -torch.eye(3, dtype=torch.float64).expand(n, 3, 3)), 2)               # (n,3,6)
        ev = e3[:, :, None]
    A = u[:, None, None] * (J.transpose(1, 2) @ J)
    b = u[:, None] * (J.transpose(1, 2) @ ev)[:, :, 0]
    S = torch.zeros(n, NACC, dtype=torch.float64)
    for i in range(6):
        for j in range(i, 6):
            S[:, tri(i, j)] = A[:, i, j]
    S[:, ACC_B:ACC_B + 6] = b
    S[:, ACC_COST] = u * (ev[:, :, 0] ** 2).sum(1)
    rows = 1.0 if pl else 3.0
    S[:, ACC_SUMW] = rows * w
    S[:, ACC_NMATCH] = rows * (w > thr).to(torch.float64)
    return torch.cat((w[:, None], S), 1)


# ---------------------------------------------------------------- the stand-alone loss weight
class LossChain:
    """loss.get_weight on err (n,r), r in 1..3, and the gradient of sum gw w (loss.py:21-58)"""

    def __init__(self, ar, name, diff, metric, tanh_k, err, flips=None, grads=True, safe=True, ieee=False, plain=False):
        self.ar = ar
        T = self.T = Tape(ar, ieee, plain)
        self.dec = {}
        self.err = err.clone().requires_grad_(grads)
        n, r = err.shape
        self.n = n
        one = torch.ones(n, dtype=torch.float64)
        dl, k = ar.par(metric), ar.par(tanh_k)
        sq = T.r(self.err * self.err, "s.p")
        s = sq[:, 0]                                    # s = 0 + e0^2 is exact
        for i in range(1, r):
            s = T.r(s + sq[:, i], "s.s%d" % i)
        en = T.r(safe_sqrt(T.flush_arg(s)), "en", c=ar.c_sqrt)
        f32 = ar.dt == F32
        if name == "huber":
            if diff:
                dl2 = T.r(torch.full((n,), dl * dl, dtype=torch.float64), "dl2")
                w = T.r(dl2 / T.r(dl2 + T.r(en * en, "en2"), "hub.den"), "lw")
            else:
                cond = _decide(self.dec, flips, "en>metric", en, dl, en.detach() > dl)
                w = T.r(torch.where(cond, dl / (torch.where(cond, en, one) if safe else en), one), "lw", mask=cond.to(torch.float64))
        elif name == "cauchy":
            t = T.r(en / dl, "cau.t")
            w = T.r(1.0 / T.r(1.0 + T.r(t * t, "cau.t2"), "cau.den"), "lw")
        elif name == "trim":
            if diff:
                w, _ = _soft_gate(T, ar, k, dl, en, "ltrim")
            else:
                w = _decide(self.dec, flips, "en<metric", en, dl, en.detach() < dl).to(torch.float64)
        else:
            raise ValueError(name)
        self.w = w
        self.extreme = T.extreme if T.extreme is not None else torch.zeros(n, dtype=torch.bool)

    def forward_outputs(self):
        return self.w[:, None]

    def backward_outputs(self, gw):
        if not self.w.requires_grad:
            return torch.zeros_like(self.err)
        (g,) = torch.autograd.grad((gw * self.w).sum(), [self.err], create_graph=True)
        return g

    def bound(self, out, backward=False):
        B = tape_bound(self.T, out, backward, self.extreme)
        if backward:        # loss_weight_bwd_kernel forms gw dw e_k BEFORE it divides by en: what that product loses below FLOOR comes back 1 / en times as large
            en = self.T.values["en"].detach()
            B = B + torch.where(en > 0, self.ar.floor / en, torch.zeros_like(en))[:, None]
        return B

    decision_bounds = Chain.decision_bounds


# ---------------------------------------------------------------- the comparator
def within(got, ref, bound):
    """elementwise: |got - ref| <= bound; a NaN is off its bound unless the reference is NaN at the same place; an infinite reference wants the
    same infinity"""
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - ref) <= bound
    ok |= np.isnan(ref) & np.isnan(got)
    ok |= np.isinf(ref) & (got == ref)
    return ok


def ratios(got, ref, bound):
    """|error| / bound where both are finite numbers (the measurement that is recorded; nothing is tuned to it)"""
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    with np.errstate(invalid="ignore", divide="ignore"):
        rt = np.abs(got - ref) / bound
    return np.where(np.isfinite(rt), rt, 0.0)


class OffBound(AssertionError):
    """check_points' refusal; .point is the first point off its bound"""

    def __init__(self, message, point):
        super().__init__(message)
        self.point = point


def check_points(got, ref, bound, what, tie=None, alts=(), families=None, record=None, skip=None, extreme=None):
    """got, ref, bound (n,K): every point's outputs within their bounds.  tie (n,) bool: such a point may instead lie within the bounds of ONE of
    alts = [(ref_alt, bound_alt), ...], wholly (all K outputs against the same alternative).  families: {name: columns}; record: {name: worst
    ratio} is updated with the largest |error| / bound over the points that are not ties."""
    got = np.asarray(got, dtype=np.float64)
    ref, bound = np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    ok = within(got, ref, bound)
    if skip is not None:
        ok |= np.asarray(skip, dtype=bool)[:, None]
    if extreme is not None:         # whether 0 * inf or inf - inf comes out as +inf, -inf or NaN hangs on values below the floor: not finite is the class
        ok |= np.asarray(extreme, dtype=bool)[:, None] & ~np.isfinite(ref) & ~np.isfinite(got)
    good = ok.all(1)
    resolved = {}
    if tie is not None and len(alts):
        tie = np.asarray(tie, dtype=bool)
        for i in np.flatnonzero(tie):
            sides = [bool(ok[i].all())] + [bool(within(got[i], ra[i], ba[i]).all()) for ra, ba in alts]
            good[i] = any(sides)
            resolved[int(i)] = sides
    if not good.all():
        i = int(np.flatnonzero(~good)[0])
        rt = ratios(got[i], ref[i], bound[i])
        k = int(np.argmax(np.where(ok[i], 0, np.maximum(rt, 1e-300))))
        raise OffBound("%s: %d of %d points off their bound; point %d%s output %d: got %r, reference %r, bound %.3g (error / bound %.4g)" % (
            what, int((~good).sum()), got.shape[0], i, " (a tie: matches neither side wholly)" if tie is not None and tie[i] else "",
            k, got[i, k], ref[i, k], bound[i, k], rt[k]), i)
    if record is not None and families is not None:
        rt = ratios(got, ref, bound)
        if tie is not None:
            rt = rt[~np.asarray(tie, dtype=bool)]
        for name, cols in families.items():
            if rt.size:
                record[name] = max(record.get(name, 0.0), float(rt[:, cols].max()))
    return resolved


FWD_FAMILIES = {"w": [0], "slots": list(range(1, 31))}
BWD_FAMILIES = {"gsrc": [0, 1, 2], "gtgt": [3, 4, 5], "gnormal": [6, 7, 8], "gw": [9], "pose": list(range(10, 22))}


# ---------------------------------------------------------------- the configuration grid and the inputs
PARAM_SETS = ((2.0, 10.0, 1.0, 0.01), (1.5, 5.0, 0.3, 0.05))        # (trim_dist, tanh_steepness, metric, match_ratio_thresh): the other tests' values, and another pair
MODES = (("pt2pt", 3), ("pt2pt", 6), ("pt2pl", 6))                  # (mode, elements per target row)


def grid():
    """every configuration: {pt2pt c=3, pt2pt c=6, pt2pl} x {none, huber, cauchy, trim} x {differentiable, hard} x {trim on, off} x PARAM_SETS"""
    out = []
    for mode, c in MODES:
        for loss in ("none", "huber", "cauchy", "trim"):
            for diff in (True, False):
                for trim_on in (True, False):
                    for ps, (tau, k, metric, thr) in enumerate(PARAM_SETS):
                        out.append(dict(mode=mode, c=c, loss=loss, diff=diff, trim_on=trim_on, trim_dist=tau, tanh_k=k, metric=metric, match_thresh=thr, ps=ps))
    return out


def cfg_id(cfg):
    return "%s-c%d-%s-%s-%s-p%d" % (cfg["mode"], cfg["c"], cfg["loss"], "diff" if cfg["diff"] else "hard", "trim" if cfg["trim_on"] else "notrim", cfg["ps"])


def rotations(n, rng, angle=0.3):
    """(n,3,3) float64 rotations by up to `angle` radians (Rodrigues)"""
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    th = rng.uniform(-angle, angle, n)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    return np.eye(3)[None] + np.sin(th)[:, None, None] * K + (1 - np.cos(th))[:, None, None] * (K @ K)


def random_points(n, dtype, seed, scale=3.0, dmax=3.0, w_init=True, dmin=0.02):
    """n independent well-conditioned points: coordinates of a few metres, residuals of 0.02 .. dmax metres (around the metrics and the trim
    distance), unit normals, weights in [0.5, 1], a small pose.  -> inp (float64 tensors of values representable in dtype)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-scale, scale, (n, 3))
    C = rotations(n, rng)
    r = rng.uniform(-0.5, 0.5, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    y = np.einsum("nij,nj->ni", C, p) + r - d * rng.uniform(dmin, dmax, (n, 1))
    nrm = d + 0.5 * rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    w = rng.uniform(0.5, 1.0, n) if w_init else np.ones(n)
    return dict(p=round_to(p, dtype), y=round_to(y, dtype), nrm=round_to(nrm, dtype), C=round_to(C, dtype), r=round_to(r, dtype),
                w_init=round_to(w, dtype), alive=torch.ones(n, dtype=torch.float64))


def random_cotangents(n, dtype, seed):
    """Gs (n,36) symmetric, gb (n,6)"""
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(n, 6, 6))
    G = round_to(G, dtype)
    G = torch.triu(G) + torch.triu(G, 1).transpose(1, 2)
    return G.reshape(n, 36).contiguous(), round_to(rng.normal(size=(n, 6)), dtype)


def take(inp, sel):
    return {k: v[sel] for k, v in inp.items()}


def cat(inps):
    return {k: torch.cat([i[k] for i in inps]) for k in inps[0]}


# ---- edge sets: built from exactly representable values so that each edge is HIT in the dtype under test (asserted on the reference alone)
def _base(n, dtype, w=1.0):
    z = torch.zeros(n, 3, dtype=torch.float64)
    nrm = z.clone()
    nrm[:, 2] = 1.0
    return dict(p=z.clone(), y=z.clone(), nrm=nrm, C=torch.eye(3, dtype=torch.float64).repeat(n, 1, 1), r=z.clone(),
                w_init=torch.full((n,), w, dtype=torch.float64), alive=torch.ones(n, dtype=torch.float64))


def _place(inp, i, p, r, resid, nrm=None):
    """point i: C = I, so C p + r - y = resid exactly when everything has few bits"""
    inp["p"][i] = torch.tensor(p, dtype=torch.float64)
    inp["r"][i] = torch.tensor(r, dtype=torch.float64)
    inp["y"][i] = inp["p"][i] + inp["r"][i] - torch.tensor(resid, dtype=torch.float64)
    if nrm is not None:
        inp["nrm"][i] = torch.tensor(nrm, dtype=torch.float64)


def _representable(inp, dtype):
    for k, v in inp.items():
        assert torch.equal(round_to(v, dtype), v), "edge input %s is not representable in %s" % (k, np_dtype(dtype))
    return inp


def edge_sets(cfg, dtype):
    """-> {name: (inp, expect)}: expect(chain) asserts on the reference that the edge is hit; placed ties are found by decision_bounds"""
    dt = np_dtype(dtype)
    tau, metric, thr = (float(np.float32(cfg[k])) if dt == F32 else cfg[k] for k in ("trim_dist", "metric", "match_thresh"))
    pl = cfg["mode"] == "pt2pl"
    sets = {}
    # 1. zero residual: C p + r == y exactly (pt2pt: d3 = 0); pt2pl: e = 0 with d3 > 0 (the residual lies in the plane)
    a = _base(4, dtype)
    _place(a, 0, [1.0, 2.0, -0.5], [0.25, -0.5, 0.125], [0.0, 0.0, 0.0])
    _place(a, 1, [0.5, -1.5, 2.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], nrm=[0.0, 1.0, 0.0])
    _place(a, 2, [1.0, 2.0, -0.5], [0.25, -0.5, 0.125], [0.25, 0.0, 0.0], nrm=[0.0, 0.0, 1.0])      # in-plane residual: e = 0, d3 = 0.25
    _place(a, 3, [-2.0, 0.5, 0.75], [0.0, 0.5, 0.0], [0.0, -0.5, 0.0], nrm=[1.0, 0.0, 0.0])

    def hit_zero(v):
        assert bool((v("d3")[:2] == 0).all())
        if pl:
            assert bool((v("e.s2") == 0).all()) and bool((v("d3")[2:] > 0).all())
    sets["zero_residual"] = (a, hit_zero)
    # 2. residual exactly the metric / the trim distance (the hard gates' placed ties; the documented 0.99999994 of a * rcp(a))
    a = _base(4, dtype)
    _place(a, 0, [1.0, 2.0, -0.5], [0.25, -0.5, 0.5], [0.0, 0.0, metric])        # (p_z + r_z = 0: y_z = -+ the value itself, representable)
    _place(a, 1, [0.5, -1.5, 2.0], [0.0, 0.0, -2.0], [0.0, 0.0, -metric])
    _place(a, 2, [1.0, 2.0, -0.5], [0.25, -0.5, 0.5], [0.0, 0.0, tau])
    _place(a, 3, [0.5, -1.5, 2.0], [0.0, 0.0, -2.0], [0.0, 0.0, -tau])

    def hit_metric(v):
        en = v("e.s2").abs() if pl else v("d3")
        assert bool((en[:2] == metric).all()) and bool((v("d3")[2:] == tau).all())
    sets["at_metric"] = (a, hit_metric)
    # 3. saturated gates, w = 0, w just above and below match_thresh
    a = _base(8, dtype)
    _place(a, 0, [1.0, 2.0, -0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 64.0])            # far beyond the trim distance: th = -1
    _place(a, 1, [1.0, 2.0, -0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 2.0 ** -10])      # far inside
    _place(a, 2, [1.0, 2.0, -0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 0.125])
    a["w_init"][2] = 0.0                                                          # w = 0: root - 1e-5 cancels
    for i, f in ((3, 1 + 2.0 ** -18), (4, 1 - 2.0 ** -18), (5, 1.0)):             # w = w_init just above / below (32 ulp in float32: held decisions where tw = lw = 1) / at match_thresh (a tie)
        _place(a, i, [1.0, 2.0, -0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0])
        a["w_init"][i] = float(np.float32(thr * f)) if dt == F32 else thr * f
    _place(a, 6, [1.0, 2.0, -0.5], [0.0, 0.0, 0.0], [0.0, 0.0, -4096.0])
    _place(a, 7, [1.0, 2.0, -0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 2.0 ** -20])

    def hit_sat(v):
        if v("trim.th") is not None:
            th = v("trim.th")
            assert float(th[0]) == -1.0 and float(th[6]) == -1.0 and float(v("trim.tw")[0]) == 0.0
        assert float(v("w")[2]) == 0.0
    sets["saturated"] = (a, hit_sat)
    # 4. tiny and huge residuals: en^2 subnormal, underflowing, overflowing in float32
    a = _base(6, dtype)
    for i, v in enumerate((1e-20, 1e-30, 1e20, -1e-20, -1e-30, -1e20)):
        v = float(np.float32(v)) if dt == F32 else v
        _place(a, i, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, v])

    def hit_tiny(v):
        if dt == F32:
            assert bool(v("extreme").any())
    sets["tiny_huge"] = (a, hit_tiny)
    # 5. far from the origin: 2.5 km and 25 km with centimetre residuals
    rng = np.random.default_rng(5)
    n = 64
    a = random_points(n, np.float64, 50, scale=1.0)
    off = np.where(np.arange(n) % 2 == 0, 2500.0, 25000.0)[:, None] * np.array([[1.0, -0.6, 0.02]])
    C = a["C"].numpy()
    p = rng.uniform(-20, 20, (n, 3)) + off
    r = rng.uniform(-0.5, 0.5, (n, 3)) + (off - np.einsum("nij,nj->ni", C, off))      # the pose keeps the far cloud where it is
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    a["C"], a["p"], a["r"] = round_to(C, dtype), round_to(p, dtype), round_to(r, dtype)
    q = np.einsum("nij,nj->ni", a["C"].numpy(), a["p"].numpy()) + a["r"].numpy()
    a["y"] = round_to(q - d * rng.uniform(0.01, 0.05, (n, 1)), dtype)
    a["nrm"], a["w_init"] = round_to(a["nrm"], dtype), round_to(a["w_init"], dtype)

    def hit_far(v):
        assert float(v("qr").abs().max()) > 2.0e4 and float(v("d3").max()) < 0.06
    sets["far_from_origin"] = (a, hit_far)
    # 6. weights: w_init of 0, 1, 1e-12, 1e6; alive = 0
    a = random_points(5, dtype, 60, dmax=residual_limit(cfg))
    for i, v in enumerate((0.0, 1.0, 1e-12, 1e6, 0.75)):
        a["w_init"][i] = float(np.float32(v)) if dt == F32 else v
    a["alive"][4] = 0.0

    def hit_w(v):
        assert float(v("w")[0]) == 0.0 and float(v("w")[4]) == 0.0
    sets["weights"] = (a, hit_w)
    for name, (a, _) in sets.items():
        _representable(a, dtype)
    return sets


def _evaluate(make, cot, hard_nan):
    """make(**kw) -> a chain.  -> (chain, forward (ref, bound), backward (ref, bound) | None): the bounds from the chain autograd can walk everywhere, the
    gradients from the reference's own torch.where where that differs (hard Huber: NaN at a zero residual), the values of a point with an intermediate
    outside the dtype's range from the evaluation that keeps +-inf"""
    ch = make(safe=True, grads=cot is not None)
    fo = ch.forward_outputs()
    fwd = [fo.detach().numpy().copy(), ch.bound(fo).numpy()]
    ext = ch.extreme.numpy()
    if ext.any():
        with torch.no_grad():
            fwd[0][ext] = make(safe=True, grads=False, ieee=True).forward_outputs().numpy()[ext]
    bwd = None
    if cot is not None:
        bo = ch.backward_outputs(*cot)
        bwd = [bo.detach().numpy().copy(), ch.bound(bo, backward=True).numpy()]
        if hard_nan:
            bwd[0] = make(safe=False, grads=True).backward_outputs(*cot).detach().numpy()
    return ch, fwd, bwd


NAN_COLUMNS = list(range(0, 6)) + list(range(10, 22))          # gsrc, gtgt and the pose sums (the normals' gradient of pt2pt is 0, gw does not pass the loss slope)


def extreme_gradients(ar, cfg, inp, cot, ch, bwd, hard_nan):
    """The gradients of the points with an intermediate outside the dtype's range (`extreme`).  Two float64 evaluations exist for them: the plain one
    (1e40 and 1e-60 fit a double) and the one with the format's replacement (an underflowed or flushed d3^2 is 0, so its square root's gradient is
    0: the term of the soft trim gate and of the loss through |e3| is DROPPED, which is what `s.d3 > T(0)` in point_backward does).  Such a point must
    lie, wholly, within the first-order bound of one of the two.  Two documented edges are pinned instead (dicp_math.h, 'Edges of the range'):
      pt2pt, hard Huber, a residual whose square underflows: en = d3 = 0, the zero-residual NaN of the reference is reached by underflow;
      pt2pt, differentiable Huber or Cauchy, a residual whose square overflows: en = inf, lw = 0 and the slope -2 en lw^2 / metric^2 is inf * 0 = NaN.
    There gsrc, gtgt and the pose sums are NaN and gw and the normals' columns are the replaced evaluation's.
    -> ((reference, bound) of the plain evaluation, pinned (n,) bool); bwd (the replaced evaluation's) gets the NaNs planted in its pinned rows"""
    plain = Chain(ar, cfg, inp, grads=True, plain=True)
    bo = plain.backward_outputs(*cot)
    r1, B1 = bo.detach().numpy().copy(), plain.bound(bo, backward=True).numpy()
    if hard_nan:
        r1 = Chain(ar, cfg, inp, grads=True, plain=True, safe=False).backward_outputs(*cot).detach().numpy().copy()
    pinned = np.zeros(ch.n, dtype=bool)
    if cfg["mode"] == "pt2pt":
        d3r, d3p = ch.T.values["d3"].detach().numpy(), plain.T.values["d3"].detach().numpy()
        if hard_nan:
            pinned |= (d3r == 0) & (d3p > 0)
        if (cfg["loss"] == "huber" and cfg["diff"]) or cfg["loss"] == "cauchy":
            pinned |= plain.T.values["d3sq.s2"].detach().numpy() > ar.fmax
    pinned &= ch.extreme.numpy()
    for arr in (bwd[0], r1):
        arr[np.ix_(pinned, NAN_COLUMNS)] = np.nan
    return (r1, B1), pinned


def reference(ar, cfg, inp, cot=None, allow_ties=False):
    """Everything the tests need for one configuration and one input:
    -> dict(fwd=(ref, bound), bwd=(ref, bound) | None, tie (n,) bool, alts_fwd, alts_bwd, extreme, decisions, chain).  The gradients of an `extreme` point are
    not held (first order says nothing there, and autograd of an evaluation with infinities is NaN throughout); its w and slots are."""
    hard_nan = cfg["loss"] == "huber" and not cfg["diff"]
    ch, fwd, bwd = _evaluate(lambda **kw: Chain(ar, cfg, inp, **kw), cot, hard_nan)
    res = dict(chain=ch, extreme=ch.extreme.numpy(), fwd=fwd, bwd=bwd)
    res["bwd_plain"], res["pinned_nan"] = None, np.zeros(ch.n, dtype=bool)
    if cot is not None and res["extreme"].any():
        res["bwd_plain"], res["pinned_nan"] = extreme_gradients(ar, cfg, inp, cot, ch, bwd, hard_nan)
    decs = ch.decision_bounds()
    tie = torch.zeros(ch.n, dtype=torch.bool)
    for name, (v, thr, t) in decs.items():
        tie |= t
    res["tie"], res["decisions"] = tie.numpy(), decs
    res["alts_fwd"], res["alts_bwd"] = [], []
    if bool(tie.any()):
        assert allow_ties, "random inputs must contain no tie: %s" % {k: int(t.sum()) for k, (_, _, t) in decs.items()}
        # every combination of the tied decisions, taken the other way on the tied points
        names = [k for k, (_, _, t) in decs.items() if bool(t.any())]
        for m in range(1, 2 ** len(names)):
            flips = {k: decs[k][2] for i, k in enumerate(names) if (m >> i) & 1}
            _, fa, ba = _evaluate(lambda **kw: Chain(ar, cfg, inp, flips=flips, **kw), cot, hard_nan)
            res["alts_fwd"].append(fa)
            if cot is not None:
                res["alts_bwd"].append(ba)
    return res


# ---------------------------------------------------------------- the g++ build of the header (tests/hostcheck), shared by the CPU tests


class WeightParams(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("trim_on", ctypes.c_int), ("differentiable", ctypes.c_int),
                ("loss", ctypes.c_int), ("trim_dist", ctypes.c_double), ("tanh_k", ctypes.c_double),
                ("loss_delta", ctypes.c_double), ("match_thresh", ctypes.c_double)]


HOSTCHECK_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "hostcheck.cpp")


def load_hostcheck():
    import hostbuild
    lib = hostbuild.build("hostcheck.cpp", "hostcheck")
    assert lib.hc_sizeof_params() == ctypes.sizeof(WeightParams)
    return lib


def params_of(cfg, cls=WeightParams):
    return cls(mode=1 if cfg["mode"] == "pt2pl" else 0, trim_on=int(cfg["trim_on"]), differentiable=int(cfg["diff"]), loss=LOSS_CODE[cfg["loss"]],
               trim_dist=cfg["trim_dist"], tanh_k=cfg["tanh_k"], loss_delta=cfg["metric"], match_thresh=cfg["match_thresh"])


def target_rows(inp, c, dt):
    """(n,c) target rows in the dtype: point, then the normal where the row has one"""
    y = inp["y"].numpy().astype(dt)
    return np.ascontiguousarray(np.concatenate((y, inp["nrm"].numpy().astype(dt)), 1) if c >= 6 else y)


def pose_rows(inp, dt):
    n = inp["p"].shape[0]
    return np.ascontiguousarray(np.concatenate((inp["C"].numpy().reshape(n, 9), inp["r"].numpy()), 1).astype(dt))


class HostBackend:
    """the g++ instantiation of point_forward / point_backward / the restated loss kernels, one point per call of the header's functions"""
    build = "host"

    def __init__(self, lib):
        self.lib = lib

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def forward(self, dtype, cfg, inp, **kw):
        dt = np_dtype(dtype)
        sfx = "f32" if dt == F32 else "f64"
        n, c = inp["p"].shape[0], cfg["c"]
        P = params_of(cfg)
        src, tgt, pose = np.ascontiguousarray(inp["p"].numpy().astype(dt)), target_rows(inp, c, dt), pose_rows(inp, dt)
        w0 = inp["w_init"].numpy().astype(dt) * inp["alive"].numpy().astype(dt)
        acc, w = np.zeros((n, NACC), dt), np.zeros(n, dt)
        getattr(self.lib, "hc_points_forward_" + sfx)(ctypes.byref(P), n, c, self._p(src), self._p(tgt), self._p(pose), self._p(w0), self._p(acc), self._p(w))
        return np.concatenate((w[:, None], acc), 1).astype(np.float64)

    def backward(self, dtype, cfg, inp, cot, **kw):
        dt = np_dtype(dtype)
        sfx = "f32" if dt == F32 else "f64"
        n, c = inp["p"].shape[0], cfg["c"]
        P = params_of(cfg)
        src, tgt, pose = np.ascontiguousarray(inp["p"].numpy().astype(dt)), target_rows(inp, c, dt), pose_rows(inp, dt)
        alive = inp["alive"].numpy().astype(dt)
        w0 = inp["w_init"].numpy().astype(dt) * alive
        Gs, gb = np.ascontiguousarray(cot[0].numpy().astype(dt)), np.ascontiguousarray(cot[1].numpy().astype(dt))
        gsrc, gtgt, gw, gpose = np.zeros((n, 3), dt), np.zeros((n, c), dt), np.zeros(n, dt), np.zeros((n, 12), dt)
        with np.errstate(all="ignore"):
            getattr(self.lib, "hc_points_backward_" + sfx)(ctypes.byref(P), n, c, self._p(src), self._p(tgt), self._p(pose), self._p(w0), self._p(Gs), self._p(gb),
                                                          self._p(gsrc), self._p(gtgt), self._p(gw), self._p(gpose))
            gw = gw * alive
        gn = gtgt[:, 3:6] if (c >= 6 and cfg["mode"] == "pt2pl") else np.zeros((n, 3), dt)
        if c >= 6 and cfg["mode"] != "pt2pl":
            assert not gtgt[:, 3:].any(), "pt2pt wrote a gradient into the normals' columns"
        return np.concatenate((gsrc, gtgt[:, :3], gn, gw[:, None], gpose), 1).astype(np.float64)

    def loss_weight(self, dtype, name, diff, metric, tanh_k, err, gw):
        dt = np_dtype(dtype)
        sfx = "f32" if dt == F32 else "f64"
        e = np.ascontiguousarray(err.numpy().astype(dt))
        g = np.ascontiguousarray(gw.numpy().astype(dt))
        rows, r = e.shape
        w, ge = np.zeros(rows, dt), np.zeros((rows, r), dt)
        L = LOSS_CODE[name]
        getattr(self.lib, "hc_loss_weight_" + sfx)(L, int(diff), ctypes.c_double(metric), ctypes.c_double(tanh_k), self._p(e), ctypes.c_long(rows), r, self._p(w))
        getattr(self.lib, "hc_loss_weight_bwd_" + sfx)(L, int(diff), ctypes.c_double(metric), ctypes.c_double(tanh_k), self._p(e), self._p(g), ctypes.c_long(rows), r, self._p(ge))
        return w.astype(np.float64), ge.astype(np.float64)


# ---------------------------------------------------------------- one configuration against one backend
SEEDS = {}          # (dtype name, cfg_id) -> seed of the random points, where the default one places a tie


def residual_limit(cfg):
    """The largest residual of a random point.  A soft gate far below 0 leaves a weight no larger than the absolute error of its tanh: the model is first
    order, and sqrt(w + 1e-10) is not linear over a perturbation of w's own size.  tanh's argument stays above -5 (tw >= 4.5e-5), which
    check_case asserts in the form it matters: B(w) <= (w + 1e-10) / 64 on every random point."""
    lim = 3.0
    if cfg["diff"] and cfg["trim_on"]:
        lim = min(lim, cfg["trim_dist"] + 2.0 / cfg["tanh_k"])
    if cfg["diff"] and cfg["loss"] == "trim":
        lim = min(lim, cfg["metric"] + 2.0 / cfg["tanh_k"])
    return lim


def run_gate_tail(backend, dtype, cfg, n=1024):
    """The region residual_limit leaves out of the first-order check: a soft gate between tanh argument -5 and exact saturation, where w is no larger than
    the absolute error of its tanh.  What holds there without linearity: the gate's weight is a rounded value of 0.5 th + 0.5 with th in [-1, 1] within
    its absolute error, so 0 <= w <= w_ref + B(w) (B is dominated by that absolute error and does not need w to be large), and every slot is finite."""
    assert cfg["diff"] and (cfg["trim_on"] or cfg["loss"] == "trim")
    ar = Arith(dtype, backend.build)
    lim = residual_limit(cfg)
    inp = random_points(n, dtype, 77, dmin=lim, dmax=lim + 4.0)
    ch = Chain(ar, cfg, inp)
    fo = ch.forward_outputs()
    w, Bw = fo.detach().numpy()[:, 0], ch.bound(fo).numpy()[:, 0]
    assert (w < 1e-3).mean() > 0.5 and (w > 0).any(), "the inputs must lie in the gate's tail"
    got = backend.forward(dtype, cfg, inp)
    assert np.isfinite(got).all()
    assert (got[:, 0] >= 0).all() and (got[:, 0] <= w + Bw).all(), "a weight in the gate's tail left [0, w_ref + B]: point %s" % np.flatnonzero(~((got[:, 0] >= 0) & (got[:, 0] <= w + Bw)))[:5]
    return float((got[:, 0] / (w + Bw)).max())


def random_case(dtype, cfg, n, seed_key=None):
    seed = SEEDS.get((np_dtype(dtype).name, seed_key or cfg_id(cfg)), 1)
    return random_points(n, dtype, seed, dmax=residual_limit(cfg)), random_cotangents(n, dtype, seed + 1000)


def config_case(dtype, cfg, n, edges=True):
    """-> (inp, cot, n random points first, [(edge name, first, count, expect)]): the random points and every edge set of a configuration as ONE batch
    (the points are independent)"""
    inp, cot = random_case(dtype, cfg, n)
    parts, cots, spans, at = [inp], [cot], [], n
    if edges:
        for name, (a, expect) in edge_sets(cfg, dtype).items():
            m = a["p"].shape[0]
            parts.append(a)
            cots.append(random_cotangents(m, dtype, 7))
            spans.append((name, at, m, expect))
            at += m
    return cat(parts), (torch.cat([c[0] for c in cots]), torch.cat([c[1] for c in cots])), n, spans


def check_case(ref, n, spans):
    """no tie among the random points; every edge is hit (on the reference alone)"""
    assert not ref["tie"][:n].any(), "random inputs must contain no tie: points %s" % np.flatnonzero(ref["tie"][:n])
    assert not ref["extreme"][:n].any()
    ch = ref["chain"]
    w, Bw = ref["fwd"][0][:n, 0], ref["fwd"][1][:n, 0]
    assert (Bw <= (w + 1e-10) / 64).all(), "random inputs must keep w out of the region where its own error is of its size: points %s" % np.flatnonzero(Bw > (w + 1e-10) / 64)
    for name, at, m, expect in spans:
        def view(key, at=at, m=m):
            if key == "extreme":
                return ch.extreme[at:at + m]
            t = ch.T.values.get(key)
            return None if t is None else t.detach()[at:at + m]
        expect(view)


def run_config(backend, dtype, cfg, n, record=None, ties_log=None, edges=True, **kw):
    """The random points (no tie) and every edge set of one configuration: the backend's w, 30 slots and gradients within the model's bounds."""
    ar = Arith(dtype, backend.build)
    what = "%s %s %s" % (backend.build, np_dtype(dtype).name, cfg_id(cfg))
    inp, cot, n, spans = config_case(dtype, cfg, n, edges)
    ref = reference(ar, cfg, inp, cot, allow_ties=True)
    check_case(ref, n, spans)
    span_of = lambda i: next((nm for nm, at, m, _ in spans if at <= i < at + m), "random")
    got = backend.forward(dtype, cfg, inp, **kw)
    gotb = backend.backward(dtype, cfg, inp, cot, **kw)
    # forward and backward of a point together: a tie, or an extreme point, must be answered one way by BOTH (output 0..30 forward, 31..52 backward)
    both = lambda f, b: (np.concatenate((f[0], b[0]), 1), np.concatenate((f[1], b[1]), 1))
    main = both(ref["fwd"], ref["bwd"])
    tie_j, alts_j = ref["tie"], [both(f, b) for f, b in zip(ref["alts_fwd"], ref["alts_bwd"])]
    if ref["bwd_plain"] is not None:                        # an extreme point's gradients: wholly the replaced or wholly the plain evaluation (extreme_gradients)
        tie_j, alts_j = tie_j | (ref["extreme"] & ~ref["pinned_nan"]), alts_j + [both(ref["fwd"], ref["bwd_plain"])]
    try:
        rj = check_points(np.concatenate((got, gotb), 1), main[0], main[1], what, tie_j, alts_j, extreme=ref["extreme"])
    except OffBound as e:
        i = e.point
        raise AssertionError("%s [%s point %d]" % (e, span_of(i), i - next((at for nm, at, m, _ in spans if at <= i < at + m), 0)))
    rf = rb = rj
    if record is not None:
        tie = ref["tie"]
        for sel, rec in ((slice(0, n), record), (slice(n, None), record.setdefault("edges", {}))):
            for g, r, fam in ((got, ref["fwd"], FWD_FAMILIES), (gotb, ref["bwd"], BWD_FAMILIES)):
                rt = ratios(g[sel], r[0][sel], r[1][sel])[~(tie[sel] | (ref["extreme"][sel] if fam is BWD_FAMILIES else False))]
                for name, cols in fam.items():
                    if rt.size:
                        rec[name] = max(rec.get(name, 0.0), float(rt[:, cols].max()))
    if ties_log is not None:
        for i in np.flatnonzero(ref["tie"]):
            which = [k for k, (_, _, t) in ref["decisions"].items() if bool(t[i])]
            ties_log.append("%s %s point %d: tie on %s; sides (as the reference, then each alternative) %s" % (
                what, span_of(i), i, " + ".join(which) or "range", rj.get(int(i))))


# ---------------------------------------------------------------- the stand-alone loss weight against one backend
def loss_inputs(dtype, r, name, diff, metric, tanh_k, n=1024):
    """err (n + edges, r) and gw: random rows (residuals on both sides of the metric; below metric + 2 / k for the soft gate, see residual_limit), then the
    edge rows: zero residual, exactly the metric (both signs), saturated (64, 2^-10), tiny and huge (1e-20, 1e-30, 1e20).  -> (err, gw, n)"""
    dt = np_dtype(dtype)
    rng = np.random.default_rng(100 + r)
    lim = min(3.0, metric + 2.0 / tanh_k) if (name == "trim" and diff) else 3.0
    d = rng.normal(size=(n, r))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    e = d * rng.uniform(0.02, lim, (n, 1))
    mt = float(np.float32(metric)) if dt == F32 else metric
    edge = np.zeros((11, r))
    for i, v in enumerate((0.0, mt, -mt, 64.0, 2.0 ** -10, 1e-20, 1e-30, 1e20, -1e-20, -1e-30, -1e20)):
        edge[i, r - 1] = v
    err = round_to(np.concatenate((e, edge)), dtype)
    return err, round_to(rng.normal(size=n + 11), dtype), n


def loss_extreme(ar, name, diff, metric, k, err, gw, ch, bref):
    """extreme_gradients for the stand-alone loss: the plain float64 evaluation of the rows whose sum of squares leaves the dtype's range, and the
    pinned rows -- hard Huber with en underflowed to 0 (the zero-residual NaN), differentiable Huber / Cauchy with en = inf (slope inf * 0):
    their whole gradient row is NaN (planted into bref and the plain reference).  -> ((reference, bound), pinned)"""
    plain = LossChain(ar, name, diff, metric, k, err, plain=True)
    bo = plain.backward_outputs(gw)
    r1 = bo.detach().numpy().copy()
    B1 = plain.bound(bo, backward=True).numpy() if bo.requires_grad else np.full(tuple(bo.shape), ar.floor)
    if name == "huber" and not diff:
        r1 = LossChain(ar, name, diff, metric, k, err, plain=True, safe=False).backward_outputs(gw).detach().numpy().copy()
    enr, enp = ch.T.values["en"].detach().numpy(), plain.T.values["en"].detach().numpy()
    pinned = np.zeros(ch.n, dtype=bool)
    if name == "huber" and not diff:
        pinned |= (enr == 0) & (enp > 0)
    if (name == "huber" and diff) or name == "cauchy":
        pinned |= enp * enp > ar.fmax
    pinned &= ch.extreme.numpy()
    for arr in (bref, r1):
        arr[pinned] = np.nan
    return (r1, B1), pinned


def run_loss(backend, dtype, r, record=None, ties_log=None):
    """dicp_loss_weight{,_bwd} (or their host restatement) on every loss of the grid, random rows and edge rows, within the model's bounds"""
    ar = Arith(dtype, backend.build)
    for name in ("huber", "cauchy", "trim"):
        for diff in (True, False):
            for (_, k, metric, _) in PARAM_SETS:
                err, gw, n = loss_inputs(dtype, r, name, diff, metric, k)
                what = "%s %s loss %s %s metric %g r %d" % (backend.build, np_dtype(dtype).name, name, "diff" if diff else "hard", metric, r)
                make = lambda **kw: LossChain(ar, name, diff, metric, k, err, **{a: b for a, b in kw.items()})
                ch = make(safe=True, grads=True)
                fo = ch.forward_outputs()
                fref, fB = fo.detach().numpy().copy(), ch.bound(fo).numpy()
                ext = ch.extreme.numpy()
                if ext.any():
                    fref[ext] = make(safe=True, grads=False, ieee=True).forward_outputs().detach().numpy()[ext]
                bo = ch.backward_outputs(gw)
                bB = ch.bound(bo, backward=True).numpy() if bo.requires_grad else np.full(tuple(bo.shape), ar.floor)
                bref = (make(safe=False, grads=True).backward_outputs(gw) if (name == "huber" and not diff) else bo).detach().numpy()
                decs = ch.decision_bounds()
                tie = np.zeros(ch.n, dtype=bool)
                for _, (_, _, t) in decs.items():
                    tie |= t.numpy()
                assert not tie[:n].any() and not ext[:n].any(), "random rows must contain no tie: %s" % what
                alts_f, alts_b = [], []
                if tie.any():
                    flips = {kk: v[2] for kk, v in decs.items()}
                    alt = LossChain(ar, name, diff, metric, k, err, flips=flips)
                    fa = alt.forward_outputs()
                    alts_f.append((fa.detach().numpy(), alt.bound(fa).numpy() if fa.requires_grad else np.full((ch.n, 1), ar.floor)))
                    ba = alt.backward_outputs(gw)
                    alts_b.append((ba.detach().numpy(), alt.bound(ba, backward=True).numpy() if ba.requires_grad else np.full(tuple(ba.shape), ar.floor)))
                w, ge = backend.loss_weight(dtype, name, diff, metric, k, err, gw)
                got = np.concatenate((w[:, None], ge), 1)
                refs = np.concatenate((fref, bref), 1)
                Bs = np.concatenate((fB, bB), 1)
                res = check_points(w[:, None], fref, fB, what + " weight", tie, alts_f, extreme=ext)
                # the gradient of an extreme row: wholly the replaced or wholly the plain float64 evaluation, or the pinned NaN (loss_extreme)
                bref = bref.copy()
                tie_b, alts_bb = tie, list(alts_b)
                if ext.any():
                    plain, pinned = loss_extreme(ar, name, diff, metric, k, err, gw, ch, bref)
                    tie_b, alts_bb = tie | (ext & ~pinned), alts_bb + [plain]
                check_points(ge, bref, bB, what + " gradient", tie_b, alts_bb)
                if record is not None:
                    keep = ~(tie | ext)
                    rt = ratios(got[keep], refs[keep], Bs[keep])
                    record["loss weight"] = max(record.get("loss weight", 0.0), float(rt[:, 0].max()))
                    record["loss weight gradient"] = max(record.get("loss weight gradient", 0.0), float(rt[:, 1:].max()))
                if ties_log is not None:
                    for i in np.flatnonzero(tie):
                        ties_log.append("%s row %d (edge %d): tie on %s; sides %s" % (what, i, i - n, " + ".join(kk for kk, v in decs.items() if bool(v[2][i])), res.get(int(i))))


# ---------------------------------------------------------------- sums over the points of a cloud (the 512-point block of dicp_accumulate)
SUM_SIZES = (2, 3, 511, 512, 513, 16384)
_SUM_CFG = {2: ("pt2pl", 6, "huber", True, True), 3: ("pt2pt", 3, "cauchy", True, False), 511: ("pt2pl", 6, "trim", False, True),
            512: ("pt2pt", 6, "huber", False, True), 513: ("pt2pl", 6, "cauchy", True, True), 16384: ("pt2pl", 6, "huber", True, True)}


def sum_config(n):
    mode, c, loss, diff, trim_on = _SUM_CFG[n]
    tau, k, metric, thr = PARAM_SETS[0]
    return dict(mode=mode, c=c, loss=loss, diff=diff, trim_on=trim_on, trim_dist=tau, tanh_k=k, metric=metric, match_thresh=thr, ps=0)


def sum_case(dtype, n):
    """Four clouds of n points against m = n // 2 + 1 target rows each (in-degree about 2): rows = [n, n - 1, 0, n] take part, alive = [1, 1, 1, 0];
    one pose and one cotangent per cloud.  -> dict of numpy arrays in the dtype for the kernels, and `inp`, `cot`, `cloud`, `point`, `row` of the points
    that take part (float64 tensors / index arrays) for the reference"""
    dt = np_dtype(dtype)
    cfg = sum_config(n)
    N, m = 4, n // 2 + 1
    rng = np.random.default_rng(SEEDS.get((dt.name, "sum%d" % n), 3))
    rows = np.array([n, n - 1, 0, n], dtype=np.int32)
    alive = np.array([1.0, 1.0, 1.0, 0.0])
    C, r = rotations(N, rng), rng.uniform(-0.5, 0.5, (N, 3))
    Y = rng.uniform(-3, 3, (N, m, 3))
    nr = rng.normal(size=(N, m, 3))
    nr /= np.linalg.norm(nr, axis=2, keepdims=True)
    idx = rng.integers(0, m, (N, n)).astype(np.int32)
    d = rng.normal(size=(N, n, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    yi = np.take_along_axis(Y, idx[:, :, None].astype(np.int64), 1)
    resid = d * rng.uniform(0.02, residual_limit(cfg), (N, n, 1))
    p = np.einsum("bji,bnj->bni", C, yi + resid - r[:, None, :])                # C^T (y + e3 - r)
    w0 = rng.uniform(0.5, 1.0, (N, n))
    Gs, gb = random_cotangents(N, dtype, 11)
    K = dict(cfg=cfg, N=N, n=n, m=m, rows=rows, src=p.astype(dt), tgt=np.concatenate((Y, nr), 2).astype(dt)[:, :, :cfg["c"]].copy(), idx=idx,
             pose=np.concatenate((C.reshape(N, 9), r), 1).astype(dt), w_init=w0.astype(dt), alive=alive.astype(dt),
             Gs=Gs.numpy().astype(dt), gb=gb.numpy().astype(dt))
    cl, pt = np.nonzero(np.arange(n)[None, :] < rows[:, None])
    f = lambda a: torch.tensor(np.asarray(a, dtype=dt).astype(np.float64))
    K["cloud"], K["point"], K["row"] = cl, pt, idx[cl, pt]
    K["inp"] = dict(p=f(p[cl, pt]), y=f(Y[cl, K["row"]]), nrm=f(nr[cl, K["row"]]), C=f(C[cl]), r=f(r[cl]), w_init=f(w0[cl, pt]), alive=f(alive[cl]))
    K["cot"] = (Gs[cl], gb[cl])
    return K


def sum_reference(ar, K, backward=True):
    """-> the per-point reference of a sum_case; no tie, w inside the model's linear region (asserted on the reference alone)"""
    ref = reference(ar, K["cfg"], K["inp"], K["cot"] if backward else None, allow_ties=False)
    check_case(ref, K["inp"]["p"].shape[0], [])
    return ref


def sums_by(keys, nkeys, terms, bounds, u):
    """sum of terms (P,K) per key with the bound of the issue: the terms' bounds plus count * u_T * sum |term|.  -> (S, B, count)"""
    S, A, Bb = (np.zeros((nkeys, terms.shape[1])) for _ in range(3))
    np.add.at(S, keys, terms)
    np.add.at(A, keys, np.abs(terms))
    np.add.at(Bb, keys, bounds)
    cnt = np.bincount(keys, minlength=nkeys)
    return S, Bb + cnt[:, None] * u * A, cnt
