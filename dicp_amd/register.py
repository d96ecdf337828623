"""Poses from explicit correspondences: the closed-form fit (align_correspondences), its residuals, and the three robust estimators on
top of it -- RANSAC over minimal samples, consensus sets around the second-order seeds of compat.py, graduated non-convexity.  match.py
holds the overview of the whole chain and re-exports every public name here.
"""
import torch

from . import _lib
from ._ops import _DT, _p
from ._pairs import _finish, _flag, _idx32, _int_in, _live_pairs, _mask_idx, _number, _pair_arguments, _pose12, _T44, _threshold
from .compat import _check_compat, _compat2_stages


class _Align(torch.autograd.Function):
    """(x (N,n,3), y (N,m,3), w (N,n)) with idx (N,n) int32 in [0, m) -> T (N,4,4): dicp_kabsch_accumulate under the identity pose, then
    dicp_kabsch_step; the backward is dicp_kabsch_step_bwd, then dicp_kabsch_bwd into zeroed gradients."""

    @staticmethod
    def forward(ctx, x, y, w, idx, rows):
        N, n, _ = x.shape
        m = y.shape[1]
        dt, dev = x.dtype, x.device
        code = _DT[dt]
        nblk = _lib.load().dicp_accumulate_blocks(n)
        pose0 = torch.zeros((N, 12), dtype=dt, device=dev)
        pose0[:, 0] = pose0[:, 4] = pose0[:, 8] = 1.0
        partials = torch.empty((N, nblk, _lib.NACC_PAD), dtype=dt, device=dev)
        pose = torch.empty((N, 12), dtype=dt, device=dev)
        cost = torch.empty((N,), dtype=dt, device=dev)
        save = torch.empty((N, _lib.KAB_SAVE), dtype=torch.float64, device=dev)
        _lib.call("dicp_kabsch_accumulate", dev, code, _p(x), _p(y), 3, _p(idx), _p(pose0), _p(w), 0, 0.0, _p(rows), N, n, m, _p(partials))
        _lib.call("dicp_kabsch_step", dev, code, _p(partials), nblk, _p(pose), _p(cost), _p(save), N)
        ctx.save_for_backward(x, y, w, idx, pose0, save)
        ctx.rows = rows
        return _T44(pose)

    @staticmethod
    def backward(ctx, gT):
        x, y, w, idx, pose0, save = ctx.saved_tensors
        N, n, _ = x.shape
        m = y.shape[1]
        dt, dev = x.dtype, x.device
        code = _DT[dt]
        gpose = _pose12(gT.contiguous())
        gacc = torch.empty((N, 16), dtype=dt, device=dev)
        _lib.call("dicp_kabsch_step_bwd", dev, code, _p(gpose), _p(save), _p(gacc), N)
        gx, gy, gw = torch.empty_like(x), torch.empty_like(y), torch.empty_like(w)
        for t in (gx, gy, gw):                              # dicp_kabsch_bwd ADDS
            _lib.call("dicp_zero", dev, _p(t), t.numel() * t.element_size())
        _lib.call("dicp_kabsch_bwd", dev, code, _p(x), _p(y), 3, _p(idx), _p(pose0), _p(w), 0, 0.0, _p(gacc), _p(ctx.rows), N, n, m, _p(gx), _p(gy), _p(gw))
        return gx, gy, gw, None, None


def align_correspondences(x, y, idx, weight=None, x_rows=None):
    """The rigid transform T (N, 4, 4) minimising sum_i w_i |C x_i + r - y_idx(i)|^2 over explicit correspondences, in closed form.

    x (n, c) / (N, n, c), y (m, c) / (N, m, c): points, float32 or float64, columns 0:3 are used.  idx (n,) / (N, n) int64 or int32: the row of
    y matched to every row of x, negative = no match (match_features' output as it is).  weight: None (1) or (n,) / (N, n) in the points'
    dtype.  x_rows: optional (N,) row counts of a padded batch.  w_i = weight_i for i < x_rows[b] with idx_i >= 0, and 0 otherwise: the points
    and the idx of such rows have no influence at all.  An idx >= m is a ValueError only when idx is a CPU tensor (no read-back from the
    device: the kernel clamps it into [0, m - 1]).  A single pair of clouds returns (4, 4).

    Gradients go to x, y (columns 0:3) and weight.

    Limits, those of the ICP loop's SVD step whose kernels these are (dicp_kabsch_accumulate / _step / _step_bwd / _bwd):
    the rotation is U diag(1, 1, det U det V) V^T, always proper; the sums are un-centred raw moments, so in float32 the accuracy far from the
    origin is that of ICP's SVD step (centre the clouds first, or use float64).  A degenerate set of pairs -- no pair, all weights zero,
    or fewer than three non-collinear pairs -- has no unique minimiser: the step kernel returns the proper rotation its SVD of the (rank-
    deficient) covariance yields, with r fitting the weighted centroids, and for no pairs at all a non-finite pose (the weights' sum is 0);
    the gradients at such a point are not meaningful.
    """
    form, on_cpu, xd, yd, idx_d, w, rows = _pair_arguments(x, y, idx, weight, x_rows, "align_correspondences")
    return _finish(form, on_cpu, [_align(xd, yd, idx_d, w, rows)], 1)[0]


def _align(xd, yd, idx_d, weight, rows):
    """align_correspondences on _pair_arguments' tensors -> T (N, 4, 4)"""
    N, n, dev = xd.shape[0], xd.shape[1], xd.device
    live = idx_d >= 0
    w = torch.ones((N, n), dtype=xd.dtype, device=dev) if weight is None else weight
    w = torch.where(live, w, torch.zeros((), dtype=xd.dtype, device=dev)).contiguous()
    idx32 = torch.where(live, idx_d, torch.zeros_like(idx_d)).to(torch.int32).contiguous()
    return _Align.apply(xd, yd, w, idx32, rows)


H_MAX = 65536           # RANSAC_H_MAX (csrc/dicp_ransac.h)
REFINE_MAX = 8


def _residuals(xd, yd, idx32, rows, pose):
    """dicp_pair_residuals on detached (N, n, 3) / (N, m, 3) points -> d2 (N, n)"""
    N, n, _ = xd.shape
    d2 = torch.empty((N, n), dtype=xd.dtype, device=xd.device)
    _lib.call("dicp_pair_residuals", xd.device, _DT[xd.dtype], _p(xd), _p(yd), _p(idx32), _p(rows), _p(pose), N, n, yd.shape[1], _p(d2))
    return d2


def _score_and_refine(x0, y0, idx_d, idx32, weight, rows, pairs, P, poses, threshold, refine, real=None):
    """The stages ransac_correspondences and consensus_correspondences share, from a cloud's hypothesis poses (N, H, 12) on (under
    torch.no_grad, on detached points): dicp_ransac_score, dicp_ransac_best, I_0 and the LO rounds -> a dict under the names of
    _ransac_stages: counts, best, best_count, pose_best, thr2, sets, accepted, round_poses, inliers.  real (N, H) bool: the hypotheses that
    exist; the counts of the others are zeroed before the choice."""
    N, n, _ = x0.shape
    dt, dev = x0.dtype, x0.device
    code = _DT[dt]
    H = poses.shape[1]
    counts = torch.empty((N, H), dtype=torch.int32, device=dev)
    _lib.call("dicp_zero", dev, _p(counts), counts.numel() * 4)
    _lib.call("dicp_ransac_score", dev, code, _p(pairs), _p(P), _p(poses), N, n, H, float(threshold), _p(counts))
    if real is not None:
        counts = torch.where(real, counts, torch.zeros((), dtype=torch.int32, device=dev)).contiguous()
    best = torch.empty((N,), dtype=torch.int32, device=dev)
    best_count = torch.empty((N,), dtype=torch.int32, device=dev)
    pose_best = torch.empty((N, 12), dtype=dt, device=dev)
    _lib.call("dicp_ransac_best", dev, code, _p(counts), _p(poses), _p(P), N, H, _p(best), _p(best_count), _p(pose_best))
    thr2 = torch.full((), float(threshold) * float(threshold), dtype=dt, device=dev)        # (the product in double, rounded once to T)
    some = (P >= 3)[:, None]
    inl = (_residuals(x0, y0, idx32, rows, pose_best) <= thr2) & some
    sets, accepted, round_poses = [inl], [], []
    minus = torch.full_like(idx_d, -1)                      # (one fill for all the rounds)
    for _ in range(int(refine)):
        pj = _pose12(_align(x0, y0, torch.where(inl, idx_d, minus), weight if weight is None else weight.detach(), rows))
        round_poses.append(pj)
        new = (_residuals(x0, y0, idx32, rows, pj) <= thr2) & some
        ok = new.sum(dim=1) >= inl.sum(dim=1)
        inl = torch.where(ok[:, None], new, inl)
        sets.append(inl)
        accepted.append(ok)
    return dict(counts=counts, best=best, best_count=best_count, pose_best=pose_best, thr2=thr2, sets=sets, accepted=accepted,
                round_poses=round_poses, inliers=inl)


def _ransac_stages(xd, yd, idx_d, weight, rows, threshold, hypotheses, seed, refine, _poses=None):
    """Every stage of ransac_correspondences on _pair_arguments' tensors, as a dict: live (N, n) bool, pairs (N, n, 6), P (N,) int32,
    index (N, n) int64, samples (N, H, 3) int32, poses (N, H, 12), counts (N, H) int32, best / best_count (N,) int32, pose_best (N, 12),
    thr2 (0-d), sets [I_0 .. I_R] of (N, n) bool, accepted [(N,) bool per round], round_poses [(N, 12) per round: T_j's pose], inliers (N, n)
    bool.  _poses (N, H, 12): the poses to
    score instead of stage 1's (samples are then -1).  Nothing is read back."""
    N, n, _ = xd.shape
    dt, dev = xd.dtype, xd.device
    H = int(hypotheses)
    with torch.no_grad():
        x0, y0 = xd.detach(), yd.detach()
        pk = _live_pairs(x0, y0, idx_d, rows)
        if _poses is None:
            poses = torch.empty((N, H, 12), dtype=dt, device=dev)
            samples = torch.empty((N, H, 3), dtype=torch.int32, device=dev)
            _lib.call("dicp_ransac_hypotheses", dev, _DT[dt], _p(pk.pairs), _p(pk.P), N, n, H, int(seed) & 0xFFFFFFFF, _p(poses), _p(samples))
        else:
            poses = _poses.to(device=dev, dtype=dt).reshape(N, H, 12).contiguous()
            samples = torch.full((N, H, 3), -1, dtype=torch.int32, device=dev)
        st = dict(live=pk.live, pairs=pk.pairs, P=pk.P, index=pk.index, samples=samples, poses=poses)
        st.update(_score_and_refine(x0, y0, idx_d, pk.idx32, weight, rows, pk.pairs, pk.P, poses, threshold, refine))
    return st


def _check_refine(refine, return_hypothesis, what):
    _int_in(refine, what, "refine", 0, REFINE_MAX)
    _flag(return_hypothesis, what, "return_hypothesis")


def ransac_correspondences(x, y, idx, threshold, hypotheses=1024, seed=None, refine=1, weight=None, x_rows=None, return_hypothesis=False):
    """A rigid transform from putative correspondences of which many are wrong: RANSAC over minimal samples of three pairs, then
    LO-RANSAC refits on the inliers -- all on the GPU, per cloud, with no read-back.

    x, y, idx, weight, x_rows: exactly as align_correspondences (single clouds or padded batches, float32 or float64, columns 0:3, idx
        int32 or int64 with negative = no match; CPU tensors are computed on the GPU and returned on the CPU).
    threshold: a finite number > 0, the inlier distance (not squared).  hypotheses: an int H in [1, 65536].  refine: an int R in [0, 8].
    seed: None or an int (its low 32 bits count); None draws one 32-bit seed on the host from torch's CPU generator.
    Anything else is a ValueError before any device work.

    Definition (hardware-independent; T the points' dtype, fma its correctly rounded fused multiply-add):
     1. Row i of cloud b is live when i < x_rows[b], idx_i >= 0, and x_i[0:3] and y_j[0:3] are finite with j = min(idx_i, m - 1).  The live
        list is the live rows in ascending i, P_b of them.
     2. The sample of hypothesis h, in 32-bit wrap-around integers (mix32: the hash of the Gumbel noise):
            kc = mix32(seed ^ cloud 0x9E3779B9), kh = mix32(kc ^ h 0x85EBCA6B), u_t = mix32(kh ^ (t 0xC2B2AE35 + 0x27D4EB2F)), t = 0, 1, 2;
            mulhi(u, q) = (u q) >> 32;  a = mulhi(u0, P);  b = mulhi(u1, P - 1), b += (b >= a);
            c = mulhi(u2, P - 2), c += (c >= min(a, b)), c += (c >= max(a, b)):  three distinct positions of the live list.
        A cloud with P < 3 has no hypotheses: best -1, best_count 0, no inliers, T_best the identity, T = align_correspondences' for no pairs.
     3. The minimal fit in double: the 18 Kabsch sums from 0, the pairs a, b, c added in that order at weight 1, then the closed form of
        align_correspondences (proper rotation, rank-deficient completion); C (row-major) and r are rounded once to T.
     4. The residual of a pair under a pose in T: q_a = fma(C_a2, x_2, fma(C_a1, x_1, fma(C_a0, x_0, r_a))), e_a = q_a - y_a, d = +0, then
        d = fma(e_a, e_a, d) for a = 0, 1, 2.  The pair is an inlier iff d <= thr2 = T((double)threshold (double)threshold); a NaN d never is.
     5. count_h = the live pairs that are inliers of pose h; best = the h with the largest count, ties to the lowest h; T_best its pose.
     6. I_0 = the inliers of T_best.  For j = 1 .. R: T_j = align_correspondences on the pairs of I_{j-1} (with weight, no gradient), I_j the
        inliers of T_j's pose in T; a cloud accepts round j iff |I_j| >= |I_{j-1}|, otherwise it keeps I_{j-1}.
        inliers = I_R and T = align_correspondences(x, y, where(inliers, idx, -1), weight, x_rows).

    Returns (T, inliers): T (N, 4, 4) or (4, 4) for a single pair of clouds, inliers (N, n) or (n,) torch.bool in the original row order;
    with return_hypothesis=True also best (N,) int32, best_count (N,) int32 and T_best (N, 4, 4), the winning minimal-sample pose.

    Gradients flow through the final fit only, to x, y and weight (align_correspondences' backward on the final inlier set); the
    decisions carry none.  Nothing is read back and no launch depends on device data: with an int seed on device tensors the call can sit
    in a captured graph.  Integer counts, no float atomics: the result is bit-reproducible.

    Kernels (libdicp_hip.so): dicp_select_rows packs the live pairs, dicp_ransac_hypotheses / _score / _best, dicp_pair_residuals.
    """
    what = "ransac_correspondences"
    _threshold(threshold, what)
    _int_in(hypotheses, what, "hypotheses", 1, H_MAX)
    _number(seed, what, "seed must be None or an int", integer=True, none_ok=True)
    _check_refine(refine, return_hypothesis, what)
    form, on_cpu, xd, yd, idx_d, w, rows = _pair_arguments(x, y, idx, weight, x_rows, what)
    if seed is None:
        seed = int(torch.randint(0, 1 << 32, (1,), dtype=torch.int64).item())       # (a CPU tensor: no device read-back)
    st = _ransac_stages(xd, yd, idx_d, w, rows, threshold, hypotheses, seed, refine)
    outs = [_align(xd, yd, _mask_idx(st["inliers"], idx_d), w, rows), st["inliers"]]
    if return_hypothesis:
        outs += [st["best"], st["best_count"], _T44(st["pose_best"])]
    return _finish(form, on_cpu, outs, 2)


def correspondence_residuals(x, y, idx, T, x_rows=None):
    """The squared residual of every correspondence under a rigid transform, by rule 4 of ransac_correspondences.

    x, y, idx, x_rows: as align_correspondences.  T: (N, 4, 4), or (4, 4) for a single pair of clouds, in the points' dtype on their device;
    its rows 0:3 are the pose.  Returns d2 (N, n) / (n,) in x's dtype: d for a live row, +inf for one that is not.  No gradient.
    """
    what = "correspondence_residuals"
    form, on_cpu, xd, yd, idx_d, _, rows = _pair_arguments(x, y, idx, None, x_rows, what, T)
    N = xd.shape[0]
    with torch.no_grad():
        d2 = _residuals(xd.detach(), yd.detach(), _idx32(idx_d, yd.shape[1]), rows, _pose12(T.detach().to(xd.device).reshape(N, 4, 4)))
    return _finish(form, on_cpu, [d2], 1)[0]


GNC_ITER_MAX = 256      # GNC_ITER_MAX (csrc/dicp_gnc.h)
GNC_TRACE = 32          # GNC_TRACE: doubles of a trace record (mu, the band count, the 18 sums, the pose)
GNC_GROWTH_MAX = 16.0
GNC_LOSSES = {"tls": _lib.GNC_TLS, "gm": _lib.GNC_GM}


def _check_gnc(threshold, loss, growth, iterations, return_info, what):
    tail = "threshold must be a finite number > 0 (with a finite square > 0)"
    _number(threshold, what, tail, 0.0, float("inf"), True, True)
    if not (0.0 < float(threshold) * float(threshold) < float("inf")):
        raise ValueError("%s: %s, got %r" % (what, tail, threshold))
    if not isinstance(loss, str) or loss not in GNC_LOSSES:
        raise ValueError('%s: loss must be "tls" or "gm", got %r' % (what, loss))
    _number(growth, what, "growth must be a finite number with 1 < growth <= %g", 1.0, GNC_GROWTH_MAX, lo_open=True, fmt=(GNC_GROWTH_MAX,))
    _int_in(iterations, what, "iterations", 1, GNC_ITER_MAX)
    _flag(return_info, what, "return_info")


def _gnc_stages(xd, yd, idx_d, weight, rows, threshold, loss, growth, iterations, trace=False):
    """The kernel side of gnc_correspondences on _pair_arguments' tensors (under torch.no_grad, on detached points), as a dict: live
    (N, n) bool, pairs (N, n, 6), u (N, n) or None and P (N,) int32 (the packed pairs and their user weights), weights_packed (N, n),
    weights (N, n) in the original row order, rounds / status (N,) int32, mu (N,) float64, pose_last (N, 12), and with trace=True
    trace (N, iterations + 1, 32) float64, zero past a cloud's last record.  One dicp_gnc_fit launch; nothing is read back."""
    N, n, _ = xd.shape
    dt, dev = xd.dtype, xd.device
    with torch.no_grad():
        pk = _live_pairs(xd.detach(), yd.detach(), idx_d, rows, None if weight is None else weight.detach())
        wp = torch.empty((N, n), dtype=dt, device=dev)
        rounds = torch.empty((N,), dtype=torch.int32, device=dev)
        status = torch.empty((N,), dtype=torch.int32, device=dev)
        mu = torch.empty((N,), dtype=torch.float64, device=dev)
        pose = torch.empty((N, 12), dtype=dt, device=dev)
        tr = torch.zeros((N, int(iterations) + 1, GNC_TRACE), dtype=torch.float64, device=dev) if trace else None
        _lib.call("dicp_gnc_fit", dev, _DT[dt], _p(pk.pairs), _p(pk.P), _p(pk.u), N, n, GNC_LOSSES[loss], float(threshold), float(growth), int(iterations),
                  _p(wp), _p(rounds), _p(status), _p(mu), _p(pose), _p(tr))
        weights = pk.unpack(wp)
    return dict(live=pk.live, pairs=pk.pairs, u=pk.u, P=pk.P, weights_packed=wp, weights=weights, rounds=rounds, status=status, mu=mu, pose_last=pose,
                trace=tr)


def gnc_correspondences(x, y, idx, threshold, loss="tls", growth=1.4, iterations=128, weight=None, x_rows=None, return_info=False):
    """A rigid transform from putative correspondences of which many are wrong, by graduated non-convexity: iteratively re-weighted
    closed-form alignment under a robust cost that starts convex and is sharpened round by round -- truncated least squares (Yang et
    al. 2020, the rotation stage of TEASER++) or Geman-McClure (Fast Global Registration).  No seed, no hypothesis count; ONE kernel
    launch, a workgroup per cloud that runs every round and takes the stopping decision on the device.

    x, y, idx, weight, x_rows: exactly as align_correspondences (single clouds or padded batches, float32 or float64, columns 0:3, idx
        int32 or int64 with negative = no match; CPU tensors are computed on the GPU and returned on the CPU).
    threshold: a finite number > 0, the inlier distance (not squared).  loss: "tls" or "gm".  growth: a finite number g, 1 < g <= 16.
    iterations: an int in [1, 256].  return_info: a bool.  Anything else is a ValueError before any device work.

    Definition (hardware-independent; everything after the packing in double on the exactly converted inputs, + - * / sqrt and
    comparisons only, no fma; c2 = threshold threshold):
     1. Live pairs: rule 1 of ransac_correspondences, and where weight is given weight_i finite and > 0.  The live pairs in ascending row
        order, P per cloud; u_p the user weight (1 without one).
     2. The fit F(w): the 18 Kabsch sums from 0 with pair p at omega_p = u_p w_p (a pair with omega_p = 0 contributes nothing), then
        the closed form of align_correspondences (proper rotation, rank-deficient completion).  The order of the sums is fixed: slot
        s = p mod 1024 adds its pairs in ascending p, then the slots are added pairwise, v_i + v_(i+off) for off = 1, 2, 4, ..., 512 -- a
        function of P alone.  The pose stays in double between rounds.
     3. The residual d_p = |C x_p + r - y_p|^2: q_a = ((C_a0 x_0 + C_a1 x_1) + C_a2 x_2) + r_a, e_a = q_a - y_a, d = (e_0^2 + e_1^2) + e_2^2;
        a d that is not finite counts as +inf and gets weight 0.
     4. Round 0: w = 1, pose = F(w), then d; dmax = the largest finite d (0 if none).  A cloud with P < 3 runs nothing: weights 0,
        rounds 0, status 3, T = align_correspondences' result for no pairs, T_last the identity.
     5. loss="tls": if 2 dmax <= c2 stop (all inliers, status 0, weights 1); else mu = c2 / (2 dmax - c2).  A round: lo = (mu / (mu + 1)) c2,
        hi = ((mu + 1) / mu) c2;  w_p = 1 for d_p <= lo, 0 for d_p >= hi, and in the band sqrt(((c2 mu) (mu + 1)) / d_p) - mu (clamped into
        [0, 1]: only a last bit);  pose = F(w), new d.  Stop after a round whose band was empty, status 0; otherwise mu = mu g.
     6. loss="gm": mu = max(1, 2 dmax / c2).  A round: t = mu c2, w_p = (t / (d_p + t))^2;  pose = F(w), new d.  Stop after the round
        run at mu = 1, status 0; otherwise mu = max(1, mu / g).
     7. Guard: a round that would leave fewer than three pairs with omega_p > 0 is not applied; the previous pose and weights stand and
        the loop stops, status 2.
     8. Cap: after `iterations` applied rounds the loop stops, status 1 (a round that meets its own stopping rule there has status 0).

    Returns (T, weights): weights (N, n) / (n,) in the points' dtype and the original row order -- the final w rounded once, exactly 0 on
    rows that are not live, never requiring grad -- and T (N, 4, 4) / (4, 4) = align_correspondences(x, y, where(weights > 0, idx, -1),
    weight weights, x_rows).  With return_info=True also rounds (N,) int32 (the applied rounds), status (N,) int32, mu (N,) float64 (the
    mu of the last applied round, 0 if none) and T_last (N, 4, 4), the kernel's own last pose rounded once.

    Gradients flow through the final fit only, to x, y and weight (align_correspondences' backward); the GNC weights are constants.
    Nothing is read back and no launch depends on device data: a call on device tensors can sit in a captured graph.  No float atomics
    in the forward: the result is bit-reproducible.

    For inlier ratios of about 30 % and up.  Below that put prune_correspondences(order=2) in front (README).

    Kernels (libdicp_hip.so): dicp_select_rows packs the live pairs, dicp_gnc_fit (csrc/gnc.hip, the rules: csrc/dicp_gnc.h).
    """
    what = "gnc_correspondences"
    _check_gnc(threshold, loss, growth, iterations, return_info, what)
    form, on_cpu, xd, yd, idx_d, w, rows = _pair_arguments(x, y, idx, weight, x_rows, what)
    st = _gnc_stages(xd, yd, idx_d, w, rows, threshold, loss, growth, iterations)
    wg = st["weights"]
    outs = [_align(xd, yd, _mask_idx(wg > 0, idx_d), wg if w is None else w * wg, rows), wg]
    if return_info:
        outs += [st["rounds"], st["status"], st["mu"], _T44(st["pose_last"])]
    return _finish(form, on_cpu, outs, 2)


MEMBERS_MIN, MEMBERS_MAX = 3, 32


def consensus_correspondences(x, y, idx, threshold, inlier_threshold=None, seeds=64, members=16, refine=1, weight=None, min_length=0.0, x_rows=None,
                              return_hypothesis=False):
    """A rigid transform from putative correspondences of which nearly all may be wrong: the hypotheses are not random triples but the
    consensus sets around the matches of the highest second-order compatibility (SC2-PCR's seeds), scored, chosen and refined by
    ransac_correspondences' own stages -- on the GPU, per cloud, with no read-back and no random numbers.

    x, y, idx, weight, x_rows: exactly as ransac_correspondences.  threshold, min_length: the compatibility relation's, as
    correspondence_compatibility.  inlier_threshold: None (threshold) or a finite number > 0: the inlier distance of rules 4-6 of
    ransac_correspondences.  seeds: an int in [1, 65536].  members: an int in [3, 32].  refine: an int in [0, 8].  Anything else is a
    ValueError before any device work.

    Definition (continues rules 6-8 of second_order_compatibility):
     9. Hypothesis h, 0 <= h < min(seeds, P), is the live pair s with rank2_s == h.  Its members are s, then the first
        min(members - 1, #{q : S(s, q) > 0}) positions q in the order S(s, q) descending, q ascending.
    10. Its pose is rule 3 of ransac_correspondences over the list: the 18 Kabsch sums in double from 0, the members added in list order
        at weight 1, the same closed form, one rounding to T.  A hypothesis that does not exist (h >= P) or has fewer than three members
        (exactly the seeds with degree2 = 0, which rank behind every other) has the identity pose and count 0, as a cloud without
        hypotheses has in ransac_correspondences: it is never chosen over a real one.
    11. From the poses on, rules 4-6 of ransac_correspondences with inlier_threshold: counts, best (ties to the lowest h), I_0, the
        `refine` LO rounds, and T = align_correspondences(x, y, where(inliers, idx, -1), weight, x_rows).  A cloud with P < 3: best -1,
        best_count 0, no inliers.

    Returns (T, inliers) as ransac_correspondences; with return_hypothesis=True also best (N,) int32, best_count (N,) int32, T_best
    (N, 4, 4) and members (N, seeds, members) int32: packed positions, -1 in the unused slots.

    Gradients flow through the final fit only, to x, y and weight.  Memory and time are second_order_compatibility's, O(n^2 / 8) bytes
    per cloud, plus seeds x degree x W words for the seed rows.  Nothing is read back, no launch depends on device data (fit for a
    captured graph), integer atomics only: bit-reproducible.

    Kernels (libdicp_hip.so): those of second_order_compatibility, dicp_compat2_seeds (a wave per hypothesis: S over the seed row's set
    bits, the member list, the fit in double), then dicp_ransac_score / _best and dicp_pair_residuals.
    """
    what = "consensus_correspondences"
    _check_compat(threshold, 0, min_length, what)
    _int_in(seeds, what, "seeds", 1, H_MAX)
    _threshold(inlier_threshold, what, "inlier_threshold", none_ok=True)
    _check_refine(refine, return_hypothesis, what)
    _int_in(members, what, "members", MEMBERS_MIN, MEMBERS_MAX)
    form, on_cpu, xd, yd, idx_d, w, rows = _pair_arguments(x, y, idx, weight, x_rows, what)
    st = _consensus_stages(xd, yd, idx_d, w, rows, threshold, threshold if inlier_threshold is None else inlier_threshold, seeds, members, refine,
                           min_length)
    outs = [_align(xd, yd, _mask_idx(st["inliers"], idx_d), w, rows), st["inliers"]]
    if return_hypothesis:
        outs += [st["best"], st["best_count"], _T44(st["pose_best"]), st["members"]]
    return _finish(form, on_cpu, outs, 2)


def _consensus_stages(xd, yd, idx_d, weight, rows, threshold, inlier_threshold, seeds, members, refine, min_length):
    """Every stage of consensus_correspondences on _pair_arguments' tensors: _compat2_stages' dict plus _score_and_refine's outputs under
    the names _ransac_stages uses.  Nothing is read back."""
    st = _compat2_stages(xd, yd, idx_d, rows, threshold, min_length, seeds=seeds, members=members)
    with torch.no_grad():
        st.update(_score_and_refine(xd.detach(), yd.detach(), idx_d, st["idx32"], weight, rows, st["pairs"], st["P"], st["poses"], inlier_threshold,
                                    refine, real=st["real"]))
    return st
