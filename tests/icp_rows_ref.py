"""ICP.icp(..., source_rows=, target_rows=[, weight=]) held to the float64 oracle: the inputs and the per-cloud reference.  Host only (torch on the
CPU, no GPU, no library); tests/test_icp_rows_ref.py shows on the reference alone that these inputs can carry the bars, tests/test_gpu_icp_rows.py
compares the library with it.

The reference is the docstring's own definition of the row counts -- "as if the clouds had been given as a list of their own lengths": for cloud b of
the padded batch, oracle.dicp_oracle.icp_batched with N = 1 on source[b, :ls[b]], target[b, :lt[b]], the weight's own entries and T_init[b], in
float64, gradients by torch autograd through the oracle.  The reference freezes a converged cloud exactly (w_init becomes 0, ws = sqrt(1e-10) - 1e-5
= 0, the step is 0: ICP.py:256-257), so a per-cloud run and the batch agree on T, pc, the statistics and the first iterations[b] entries of every
history.  An (N,1) weight is a (1,1) w_init: its matched_ratio is the matched COUNT (ICP.py:248,269 sum over dim 1 of a one-column tensor).

(The oracle is handed the cloud TWICE, the second copy detached, and the first result is taken.  The clouds of a batch do not see each other, so this
is the N = 1 call -- except for torch.matrix_exp, whose path for a single matrix is off by up to 7e-11 from exp(delta^) when the 1-norm of delta^
lies just below 0.0499, while its path for a batch, the one the reference's batched loop takes, agrees with Rodrigues' formula to 3e-16.  A cloud
that is still under way takes such steps, and 7e-11 in C is 1e-9 in the next step: more than the whole 1e-10 bar, spent by the checker.)

One batch of 8 clouds, padded to n = 320 source and m = 400 target rows.  The counts sit on the edges of the wave (64), of the block (256) and of
the loop's 128-row units, each at the edge and one past it, plus one full-width and one small cloud.  Every cloud is drawn by make_pairs AT its own
size (its source rows are picks of its own target rows): a cloud cut out of a longer one loses the counterparts of most of its rows, and a 9-row
pt2pl cloud cut that way took a first step of 1.8e3 -- hence also the smallest cloud's 33 rows, and the conditioning bar of the CPU test.

The pads are built to be noticed:
  source   NaN in some clouds, 1e30 in some, copies of the cloud's own first rows in the rest (a copy that took part would shift counts and sums)
  target   NaN in some clouds; in the others the cloud's own source points moved by the TRUE pose (such a row would win the argmin if it were scored)
  weight   1.0 in some clouds, NaN in the others
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from dicp_amd.synthetic import _rot, make_pairs
from oracle import dicp_oracle as O

N, N_PAD, M_PAD = 8, 320, 400
LS = [320, 257, 256, 129, 128, 65, 64, 33]
LT = [400, 129, 385, 257, 128, 65, 400, 64]
SEED = 77
SRC_PAD = ["none", "nan", "big", "copy", "nan", "copy", "big", "copy"]        # (cloud 0 is full width: it has no pad)
TGT_PAD = ["none", "moved", "nan", "moved", "nan", "moved", "none", "nan"]
W_PAD = ["none", "nan", "one", "one", "nan", "nan", "one", "nan"]
TANH_STEEPNESS = 5.0                                                          # dicp_amd/config/dICP_config.yaml, ICP.py:119
TARGET_PAD_VAL = 1000.0
MARGIN = 1e-4                                                                 # tests/test_gpu_parity.py: a float32 run may take the other side of a hard decision this close

# One scenario of the call: everything the oracle is told.  mode: "const" (const_iter, K iterations; `tol` then only decides the "converged" flag) |
# "tol" (stop at `tol`, at most K).
# weight: "none" | "point" (N,n), zeros and values on both sides of 0.3 | "cloud" (N,1) (pt2pl only, ICP.py:508-509)
Case = namedtuple("Case", "icp_type diff dim loss trim mode thresh weight K tol")
K_ITERS, TOL = 8, 1e-4
LOSSES = {"none": None, "huber": {"name": "huber", "metric": 1.0}, "cauchy": {"name": "cauchy", "metric": 0.5}, "trim": {"name": "trim", "metric": 2.0}}


def case(icp_type="pt2pl", diff=True, dim=3, loss="huber", trim=5.0, mode="const", thresh=0.0, weight="none", K=K_ITERS, tol=TOL):
    return Case(icp_type, diff, dim, loss, trim, mode, thresh, weight, K, tol)


CASES = {
    "pl-diff-3-huber-trim-const-t0-none": case(),
    "pl-diff-3-huber-trim-tol-t0.3-point": case(mode="tol", thresh=0.3, weight="point"),
    "pl-diff-3-cauchy-trim-const-t0.3-cloud": case(loss="cauchy", thresh=0.3, weight="cloud", tol=3e-4),
    "pl-diff-3-none-notrim-tol-t0-cloud": case(loss="none", trim=None, mode="tol", weight="cloud"),
    "pl-hard-2-huber-trim-const-t0.3-point": case(diff=False, dim=2, thresh=0.3, weight="point"),
    "pl-hard-3-trim-notrim-tol-t0-none": case(diff=False, loss="trim", trim=None, mode="tol"),
    "pt-diff-3-trim-trim-tol-t0.3-point": case(icp_type="pt2pt", loss="trim", mode="tol", thresh=0.3, weight="point"),
    "pt-diff-2-cauchy-trim-const-t0.3-none": case(icp_type="pt2pt", dim=2, loss="cauchy", thresh=0.3, K=4, tol=2.7e-4),      # (flattened clouds converge linearly: steps in every decade)
    "pt-hard-3-none-notrim-const-t0-point": case(icp_type="pt2pt", diff=False, loss="none", trim=None, weight="point", tol=1e-5),
    "pt-hard-3-huber-trim-tol-t0-none": case(icp_type="pt2pt", diff=False, mode="tol"),
}


def true_pose(b):
    """The motion make_pairs planted in cloud b (it does not return it): its own draws, in its own order -> (C (3,3), r (3))."""
    n, m = LS[b], LT[b]
    g = torch.Generator().manual_seed(100000 * SEED + b)
    torch.rand((m, 3), generator=g, dtype=torch.float64)
    torch.randn((m, 3), generator=g, dtype=torch.float64)
    torch.randint(0, m, (n,), generator=g)
    torch.randn((n, 3), generator=g, dtype=torch.float64)
    axis = torch.randn(3, generator=g, dtype=torch.float64)
    ang = float(torch.rand(1, generator=g, dtype=torch.float64)) * 0.05
    trans = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 2.0 * 0.3
    return _rot(axis, ang), trans


def _twist(v):
    """(6) -> (4,4): rotation exp(v[:3]^) and translation v[3:]"""
    ang = float(v[:3].norm())
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = _rot(v[:3], ang) if ang > 0 else torch.eye(3, dtype=torch.float64)
    T[:3, 3] = v[3:]
    return T


# how far from the planted pose each cloud starts, as a fraction of it: 1 = at the identity (the whole motion to find), 0 = at the solution.
# Tolerance mode wants clouds that converge early, late and never within K_ITERS iterations.
START = [1.0, 0.0, 1.0, 0.02, 1.0, 0.3, 0.0, 1.0]
KICK = [0.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 13.0]           # ... and a start beyond the identity, in units of the planted motion, for the clouds that must not converge


@functools.lru_cache(maxsize=None)
def batch():
    """-> dict of float64 CPU tensors: source (N,320,3), target (N,400,6), T_init (N,4,4), w_point (N,320), w_cloud (N,1), gT (N,4,4), gpc (N,320,3)
    (the cotangents of the tests' loss sum(T gT) + sum over a cloud's own rows of pc gpc).  Treat as read-only."""
    g = torch.Generator().manual_seed(SEED)
    src = torch.empty((N, N_PAD, 3), dtype=torch.float64)
    tgt = torch.empty((N, M_PAD, 6), dtype=torch.float64)
    T0 = torch.empty((N, 4, 4), dtype=torch.float64)
    w_point = torch.empty((N, N_PAD), dtype=torch.float64)
    for b in range(N):
        n, m = LS[b], LT[b]
        s, t = make_pairs(1, n, m, seed=SEED, dtype=torch.float64, first=b)
        C, r = true_pose(b)
        moved = s[0] @ C.T + r                                  # the source under the planted pose: each row within the noise of a target row
        src[b, :n], tgt[b, :m] = s[0], t[0]
        if SRC_PAD[b] == "copy":
            src[b, n:] = s[0][torch.arange(N_PAD - n) % n]
        elif SRC_PAD[b] != "none":
            src[b, n:] = float("nan") if SRC_PAD[b] == "nan" else 1e30
        if TGT_PAD[b] == "moved":
            rows = torch.arange(M_PAD - m) % n
            tgt[b, m:, :3] = moved[rows]
            tgt[b, m:, 3:] = torch.tensor([0.6, 0.0, 0.8], dtype=torch.float64)
        elif TGT_PAD[b] == "nan":
            tgt[b, m:] = float("nan")
        # the start: the planted pose's twist scaled by START (+ KICK), so T_init = the solution for 0 and the identity for 1
        ax = torch.randn(3, generator=g, dtype=torch.float64)
        tw = torch.cat((ax / ax.norm() * 0.05, (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 0.6))
        Tt = torch.eye(4, dtype=torch.float64)
        Tt[:3, :3], Tt[:3, 3] = C, r
        T0[b] = _twist(KICK[b] * tw) @ _blend(Tt, 1.0 - START[b])
        # per-point weights: a tenth exactly 0, the rest in [0.05, 0.25] or [0.35, 1] -- both sides of match_ratio_thresh = 0.3, 0.05 clear of it
        u = torch.rand(N_PAD, generator=g, dtype=torch.float64)
        v = torch.rand(N_PAD, generator=g, dtype=torch.float64)
        w = torch.where(u < 0.3, 0.05 + 0.2 * v, 0.35 + 0.65 * v)
        w = torch.where(u < 0.1, torch.zeros_like(w), w)
        if W_PAD[b] != "none":
            w[n:] = float("nan") if W_PAD[b] == "nan" else 1.0
        w_point[b] = w
    w_cloud = torch.tensor([1.0, 0.7, 0.2, 0.5, 1.0, 0.9, 0.25, 0.6], dtype=torch.float64).reshape(N, 1)
    sign = lambda shape: (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(torch.float64)            # noqa: E731
    gT = (torch.rand((N, 4, 4), generator=g, dtype=torch.float64) + 0.5) * sign((N, 4, 4))
    gpc = (torch.rand((N, N_PAD, 3), generator=g, dtype=torch.float64) + 0.5) * sign((N, N_PAD, 3)) * 0.1
    return dict(source=src, target=tgt, T_init=T0, w_point=w_point, w_cloud=w_cloud, gT=gT, gpc=gpc)


def _blend(T, f):
    """the fraction f of the rigid motion T (its rotation angle and its translation scaled)"""
    C = T[:3, :3]
    ang = math.acos(max(-1.0, min(1.0, (float(C.trace()) - 1.0) / 2.0)))
    out = torch.eye(4, dtype=torch.float64)
    if ang > 0:
        axis = torch.stack((C[2, 1] - C[1, 2], C[0, 2] - C[2, 0], C[1, 0] - C[0, 1]))
        out[:3, :3] = _rot(axis, f * ang)
    out[:3, 3] = f * T[:3, 3]
    return out


def weight_of(c, data=None):
    """The weight argument of a case: None | (N,320) | (N,1)"""
    data = batch() if data is None else data
    return {"none": None, "point": data["w_point"], "cloud": data["w_cloud"]}[c.weight]


def oracle_kw(c):
    return dict(icp_type=c.icp_type, differentiable=c.diff, max_iterations=c.K, tolerance=c.tol, trim_dist=c.trim,
                loss_fn=LOSSES[c.loss], dim=c.dim, const_iter=(c.mode == "const"), tanh_steepness=TANH_STEEPNESS, match_ratio_thresh=c.thresh)


def _w_init(c, w, rows):
    """What ICP.batch_size_handling hands the loop for `rows` source rows (ICP.py:360-446, 508-509): ones for no weight, x3 along dim 1 for pt2pt"""
    w = torch.ones((1, rows), dtype=torch.float64) if w is None else w
    return w.repeat_interleave(3, dim=1) if c.icp_type == "pt2pt" else w


def _margins(c, rec, src, tgt, w0, hist_w):
    """The smallest distance of any row, at any iteration, from a hard decision of the float64 run -- tests/test_gpu_parity.py::hard_branch_margins, extended
    by the count threshold |w - match_ratio_thresh| -> dict of floats.  (A row whose given weight is exactly 0 has weight exactly 0 in every precision:
    no rounding moves it across a threshold >= 0, so it is left out of the count margin; so is a weight that IS exactly 0 or 1, which the hard
    where() branches produce exactly on either side.)"""
    if c.dim == 2:                                      # the loop ran on the planar copies (ICP.py:107-116)
        src = src * torch.tensor([1.0, 1.0, 0.0], dtype=torch.float64)
        tgt = tgt * torch.tensor([1.0, 1.0, 0.0, 1.0, 1.0, 0.0], dtype=torch.float64)[:tgt.shape[2]]
    out = dict(argmin=math.inf, trim=math.inf, loss=math.inf, count=math.inf)
    metric = LOSSES[c.loss]["metric"] if LOSSES[c.loss] is not None else None
    for idx, C, r in zip(rec["idx"], rec["C"], rec["r"]):
        ps = src @ C.transpose(1, 2) + r.reshape(-1, 1, 3)
        _, best, second = O.knn_exact_f64(ps, tgt)
        if tgt.shape[1] > 1:
            out["argmin"] = min(out["argmin"], float((second - best).min()))
        nb = torch.gather(tgt, 1, idx.unsqueeze(-1).expand(-1, -1, tgt.shape[2]))
        e3 = ps - nb[:, :, :3]
        d3 = e3.norm(dim=2)
        en = (e3 * nb[:, :, 3:]).sum(-1).abs() if c.icp_type == "pt2pl" else d3
        if not c.diff and c.trim is not None:
            out["trim"] = min(out["trim"], float((d3 - c.trim).abs().min()))
        if not c.diff and c.loss in ("huber", "trim"):
            out["loss"] = min(out["loss"], float((en - metric).abs().min()))
    live = (w0.reshape(-1) != 0)
    if live.numel() == 1:                               # one weight per cloud
        live = live.expand(hist_w.shape[1])
    ww = hist_w[:, live]
    ww = ww[(ww != 0) & (ww != 1)]
    if ww.numel():
        out["count"] = float((ww - c.thresh).abs().min())
    if bool(live.any()):
        out["count"] = min(out["count"], float((w0.reshape(-1)[w0.reshape(-1) != 0] - c.thresh).abs().min()))
    return out


def run_cloud(c, b, data=None):
    """The reference for cloud b of the batch under case c -> dict: T (4,4), pc (ls,3), deltas (k,6,1), costs (k,1), weights (k,ls*r,1), converged, iterations,
    matched_ratio, grad_source (ls,3), grad_target (lt,3|6), grad_weight (ls) | (1) | None, grad_T_init (4,4), cond (k) of the recorded normal matrices,
    steps (k) the recorded step norms, margins (dict).  k = the cloud's own iterations."""
    data = batch() if data is None else data
    n, m = LS[b], LT[b]
    cols = 6 if c.icp_type == "pt2pl" else 3
    s = data["source"][b:b + 1, :n].clone().requires_grad_(True)
    t = data["target"][b:b + 1, :m, :cols].clone().requires_grad_(True)
    T0 = data["T_init"][b:b + 1].clone().requires_grad_(True)
    wa = weight_of(c, data)
    w = None if wa is None else (wa[b:b + 1, :n] if c.weight == "point" else wa[b:b + 1]).clone().requires_grad_(True)
    rec = {}
    twice = lambda x: torch.cat((x, x.detach()))            # noqa: E731  (see the module's docstring: the cloud and a detached copy of it)
    out = O.icp_batched(twice(s), twice(t), twice(T0), twice(_w_init(c, w, n)), record=rec, **oracle_kw(c))
    rec = {k: [x[:1] for x in v] for k, v in rec.items()}
    ((out["T"][0] * data["gT"][b]).sum() + (out["pc"][0] * data["gpc"][b, :n]).sum()).backward()
    A = torch.stack(rec["A"])[:, 0]
    res = dict(T=out["T"][0], pc=out["pc"][0], deltas=out["deltas"][0], costs=out["costs"][0], weights=out["weights"][0],
               converged=bool(out["stats"]["converged"][0]), iterations=float(out["stats"]["iterations"][0]), matched_ratio=float(out["stats"]["matched_ratio"][0]),
               grad_source=s.grad[0], grad_target=t.grad[0], grad_weight=None if w is None else w.grad[0], grad_T_init=T0.grad[0],
               cond=torch.linalg.cond(A), steps=torch.stack(rec["delta"])[:, 0, :, 0].norm(dim=1))
    w0 = torch.ones(n, dtype=torch.float64) if w is None else w.detach()[0]
    hist = out["weights"][0, :, :, 0].detach()
    res["margins"] = _margins(c, rec, s.detach(), t.detach(), w0, hist[:, ::3] if c.icp_type == "pt2pt" else hist)
    return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The per-cloud references of CASES[name], computed once per process and shared: a list of N run_cloud results.  Treat as read-only."""
    return [run_cloud(CASES[name], b) for b in range(N)]


def margin(ref_b):
    return min(ref_b["margins"].values())


def float32_held(name):
    """Clouds of a case whose float64 run stays more than MARGIN away from every hard decision: the ones a float32 run is compared on -> bool (N)"""
    return np.array([margin(r) > MARGIN for r in reference(name)])


def reference_padding(c, data=None):
    """The batch as the REFERENCE pads a list of these clouds (ICP.py:386-398, 460, 472-477): zero source rows of weight 0, target rows that are copies of
    one far point, max(source) * target_pad_val -> (source, target, w_init) for the oracle's batched call."""
    data = batch() if data is None else data
    cols = 6 if c.icp_type == "pt2pl" else 3
    src = torch.zeros((N, N_PAD, 3), dtype=torch.float64)
    w = torch.zeros((N, N_PAD), dtype=torch.float64)
    wa = weight_of(c, data)
    for b in range(N):
        src[b, :LS[b]] = data["source"][b, :LS[b]]
        w[b, :LS[b]] = 1.0 if wa is None else (wa[b, :LS[b]] if c.weight == "point" else wa[b, 0])
    far = float(src.max()) * TARGET_PAD_VAL
    tgt = torch.full((N, M_PAD, cols), far, dtype=torch.float64)
    for b in range(N):
        tgt[b, :LT[b]] = data["target"][b, :LT[b], :cols]
    return src, tgt, (w.repeat_interleave(3, dim=1) if c.icp_type == "pt2pt" else w)
