"""Descriptor matching: exact nearest neighbours in feature space, the matching rules on top of them, and the closed-form rigid fit of the
matched points -- where ICP's T_init comes from.

    from dicp_amd.match import knn_features, match_features, align_correspondences
    idx, d2 = match_features(fx, fy, mutual=True, ratio=0.8)        # the accepted row of fy for every row of fx, -1 where rejected
    T0 = align_correspondences(x, y, idx)                           # (N, 4, 4): the weighted Procrustes fit of x_i -> y_idx(i)
    out = ICP(icp_type="pt2pt").icp(x, y, T_init=T0)
    T0, inliers = ransac_correspondences(x, y, idx, threshold=0.05) # ... the same fit when many of the matches are wrong (RANSAC)

The hard decisions above carry no gradient.  The soft form does: every row of fx gets the softmax-weighted mean of the target's points,
and the same closed-form fit then makes the pose differentiable in both descriptor tables:

    soft, idx, prob = soft_match_features(fx, fy, y, temperature=0.1, return_best=True)
    T0 = align_correspondences(x, soft, torch.arange(n).expand(N, n), weight=prob)

All on the GPU (libdicp_hip.so: dicp_knn_features / _backward / _backward_det, dicp_soft_match / _backward, dicp_ransac_hypotheses /
_score / _best, dicp_pair_residuals, dicp_compat_scores / _rank, dicp_compat2_bits / _common / _rank / _seeds, and the Kabsch kernels of the ICP loop), without the (n, m) distance
matrix; nothing is read back from the device.

Between the matcher and RANSAC sits the pruning step for matches of which most are wrong (spatial compatibility, spectral matching):

    idx_kept, score = prune_correspondences(x, y, idx, threshold=0.05, keep=256)    # the matches that keep their lengths to each other
    T0, inliers = ransac_correspondences(x, y, idx_kept, 0.15, hypotheses=256)      # ... need far fewer hypotheses

When only a handful of the matches are right, the second-order measure (SC2: triangles of compatible matches, on packed adjacency bits)
separates them in one pass, and its best matches seed the hypotheses instead of random triples:

    score2, degree2, degree = second_order_compatibility(x, y, idx, threshold=0.05)
    idx_kept, score2 = prune_correspondences(x, y, idx, threshold=0.05, keep=256, order=2)
    T0, inliers = consensus_correspondences(x, y, idx, threshold=0.05, seeds=64, members=16)

Without hypotheses at all, for inlier ratios of about 30 % and up: graduated non-convexity, one launch with a workgroup per cloud

    T0, weights = gnc_correspondences(x, y, idx, threshold=0.05, loss="tls")        # or loss="gm"; dicp_gnc_fit

This module holds descriptor space (knn_features, soft_match_features, match_features).  The poses are in register.py, the pruning in
compat.py, what those two share in _pairs.py; every public name of theirs is importable from here.
"""
import torch

from . import _clouds, _lib
from ._clouds import ROW, K_MIN, K_MAX, _check_deterministic
from ._ops import _DT, _p
from ._pairs import _flag, _number
from .group import _invert
from .compat import ITER_MAX, N2_MAX, correspondence_compatibility, prune_correspondences, second_order_compatibility      # noqa: F401
from .compat import _compat_stages      # noqa: F401  (the GPU suites drive the stage functions through this module, as they always have)
from .register import _consensus_stages, _gnc_stages, _pair_arguments, _ransac_stages      # noqa: F401
from .register import (GNC_GROWTH_MAX, GNC_ITER_MAX, GNC_LOSSES, GNC_TRACE, H_MAX, MEMBERS_MAX, MEMBERS_MIN, REFINE_MAX,      # noqa: F401
                       align_correspondences, consensus_correspondences, correspondence_residuals, gnc_correspondences, ransac_correspondences)

D_MAX = 256             # MATCH_D_MAX (csrc/dicp_match.h)
BWD_MFMA_D = 128        # SOFT_BWD_MFMA_D (csrc/softmatch.hip): the widest table the matrix-core backward of soft_match_features takes
FORMS = {None: _lib.MATCH_AUTO, "valu": _lib.MATCH_VALU, "mfma": _lib.MATCH_MFMA}


class _KnnFeatures(torch.autograd.Function):
    """(fx (N,n,D), fy (N,m,D)) -> (d2 (N,n,k), idx (N,n,k) int64): one library call per direction on the current stream."""

    @staticmethod
    def forward(ctx, x, y, rx, ry, k, form, det):
        N, n, D = x.shape
        m = y.shape[1]
        dt, dev = _DT[x.dtype], x.device
        need = _lib.load().dicp_knn_features_workspace_bytes(dt, N, m)
        d2 = torch.empty((N, n, k), dtype=x.dtype, device=dev)
        idx = torch.empty((N, n, k), dtype=torch.int64, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.call("dicp_knn_features", dev, dt, _p(x), _p(rx), n, _p(y), _p(ry), m, D, N, k, form, _p(d2), _p(idx), _p(ws), need)
        ctx.save_for_backward(x, y, idx)
        ctx.ry, ctx.det = ry, det
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)
        return d2, idx

    @staticmethod
    def backward(ctx, g_d2, _g_idx):
        want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g_d2 is None or not (want_x or want_y):
            return (None,) * 7
        x, y, idx = ctx.saved_tensors
        N, n, D = x.shape
        m, k = y.shape[1], idx.shape[2]
        dt, dev = _DT[x.dtype], x.device
        g_d2 = g_d2.contiguous()
        gx = torch.empty_like(x) if want_x else None
        gy = torch.empty_like(y) if want_y else None
        if ctx.det:                                         # the x-gradient from the same kernel (grad_y = NULL), the y-gradient stored once
            if want_x:
                _lib.call("dicp_knn_features_backward", dev, dt, _p(g_d2), _p(idx), _p(x), _p(y), n, m, D, N, k, _p(gx), None)
            if want_y:
                off, slots = _invert(idx, ctx.ry, m)
                _lib.call("dicp_knn_features_backward_det", dev, dt, _p(g_d2), _p(idx), _p(ctx.ry), _p(x), _p(y), n, m, D, N, k, _p(off), _p(slots), _p(gy))
        else:
            if want_y:
                _lib.call("dicp_zero", dev, _p(gy), gy.numel() * gy.element_size())
            _lib.call("dicp_knn_features_backward", dev, dt, _p(g_d2), _p(idx), _p(x), _p(y), n, m, D, N, k, _p(gx), _p(gy))
        return gx, gy, None, None, None, None, None


def _check_form(form, fx, what):
    """the private _form of knn_features -> the library's code; fx: the caller's argument, looked at for its dtype only"""
    if form not in FORMS:
        raise ValueError('%s: _form must be None, "valu" or "mfma", got %r' % (what, form))
    first = fx[0] if isinstance(fx, (list, tuple)) and fx else fx
    if form == "mfma" and isinstance(first, torch.Tensor) and first.dtype != torch.float32:
        raise ValueError('%s: _form="mfma" needs float32, got %s' % (what, first.dtype))
    return FORMS[form]


def knn_features(fx, fy, k=1, x_rows=None, y_rows=None, deterministic=False, _form=None):
    """The k nearest rows of fy for every row of fx in descriptor space, exactly, with gradients of the squared distances.

    fx, fy: one table each (n, D) and (m, D); a padded batch each (N, n, D) and (N, m, D) with optional integer row counts x_rows / y_rows
        (N,); or two lists of N tables.  Both in the same form, dtype (float32 or float64) and device, with the same D in [1, 256]; every
        column takes part.  CPU tensors are computed on the GPU and returned on the CPU.
    k: an int in [1, 32].  deterministic: a bool (anything else is a ValueError before any device work); see "Gradients".

    Definition (hardware-independent; fma is the correctly rounded fused multiply-add of the inputs' dtype T, the channels c ascending):
        h_j = T(0.5) q_j,  q = +0,  q = fma(y_jc, y_jc, q);        score(i, j): s = h_j,  s = fma(-x_ic, y_jc, s).
    The candidates of query i of cloud b are the rows j < y_rows[b] whose score is finite: a row of either side with a non-finite channel has
    no finite score, so it is nobody's neighbour and as a query gets none.  The result is the first k_eff = min(k, #candidates) candidates in
    (score, index) order, and the slots stay in that order.  The returned d2 is recomputed for the winners only, r = +0, t = x_ic - y_jc,
    r = fma(t, t, r): non-negative, exactly 0 for identical rows, free of the cancellation of |x|^2 + |y|^2 - 2 x.y.  Its order can differ from
    the score's order at rounding level: d2 need not ascend over the slots in its last bits.  Slots beyond k_eff, and query rows at or past
    x_rows[b], hold d2 = +inf and idx = -1, so the output feeds group_points / pool_neighbors / invert_neighbors unchanged.

    Returns (d2, idx): (n, k) for single tables, (N, n, k) for a batch, lists of (n_b, k) for lists; d2 in fx's dtype, idx int64.

    float32 runs on the matrix cores (v_mfma_f32_32x32x2_f32, whose result is the same fma chain), float64 on the vector unit; the private
    _form ("valu" / "mfma") selects the float32 kernel for cross-checks: both give the same bits.

    Gradients flow from d2 only.  The term of slot (i, s) naming row j is t_c = (T)(2 g_is (x_ic - y_jc)), formed in float64 and rounded once; an
    entry with g == 0 or idx < 0 has none.  The gradient of fx[i, c] is the sum of the query's terms in slot order from +0, written once
    (bit-reproducible); that of fy[j, c] the sum of -t_c, by default added with float atomics (the last bits can differ from run to run;
    rows nobody names get 0).  With deterministic=True the forward and the fx-gradient are the default call's, bit for bit, and the
    fy-gradient is summed per row over its list in the inverted index of the returned idx (group.invert_neighbors, built once inside the
    backward and only when fy needs a gradient), in chunks of 64 list positions -- each from +0, the partials added in order, a single chunk as
    it is; every element is stored once: no zero fill, no atomics.
    """
    _clouds._check_k(k, "knn_features", K_MIN, K_MAX)
    _check_deterministic(deterministic, "knn_features")
    code = _check_form(_form, fx, "knn_features")
    form, on_cpu, lens, n, _, xb, yb, rx, ry = _clouds.pair_features(fx, fy, x_rows, y_rows, "knn_features", D_MAX)
    d2, idx = _KnnFeatures.apply(xb, yb, rx, ry, k, code, deterministic)
    return _clouds.restore(form, on_cpu, n, lens, [(ROW, d2), (ROW, idx)])


C_MAX = 8               # SOFT_C_MAX (csrc/dicp_softmatch.h)


class _SoftMatch(torch.autograd.Function):
    """(fx (N,n,D), fy (N,m,D), values (N,m,C)) -> (out (N,n,C), idx (N,n) int64, prob (N,n)): one library call per direction on the
    current stream; lse (N,n) is kept for the backward."""

    @staticmethod
    def forward(ctx, x, y, v, rx, ry, tau, form):
        N, n, D = x.shape
        m, C = y.shape[1], v.shape[2]
        dt, dev = _DT[x.dtype], x.device
        need = _lib.load().dicp_soft_match_workspace_bytes(dt, N, m)
        out = torch.empty((N, n, C), dtype=x.dtype, device=dev)
        lse = torch.empty((N, n), dtype=x.dtype, device=dev)
        idx = torch.empty((N, n), dtype=torch.int64, device=dev)
        prob = torch.empty((N, n), dtype=x.dtype, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.call("dicp_soft_match", dev, dt, _p(x), _p(rx), n, _p(y), _p(ry), m, D, N, _p(v), C, tau, form, _p(out), _p(lse), _p(idx), _p(prob), _p(ws), need)
        ctx.save_for_backward(x, y, v, out, lse)
        ctx.rx, ctx.ry, ctx.tau, ctx.form = rx, ry, tau, form
        ctx.mark_non_differentiable(idx, prob)
        ctx.set_materialize_grads(False)
        return out, idx, prob

    @staticmethod
    def backward(ctx, g, _g_idx, _g_prob):
        want = ctx.needs_input_grad[:3]
        if g is None or not any(want):
            return (None,) * 7
        x, y, v, out, lse = ctx.saved_tensors
        N, n, D = x.shape
        m, C = y.shape[1], v.shape[2]
        dt, dev = _DT[x.dtype], x.device
        g = g.contiguous()
        gx, gy, gv = (torch.empty_like(t) if w else None for t, w in zip((x, y, v), want))      # every element is stored by the kernels
        need = _lib.load().dicp_soft_match_workspace_bytes(dt, N, m)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        form = _lib.MATCH_AUTO if ctx.form == _lib.MATCH_MFMA and D > BWD_MFMA_D else ctx.form        # (wider tables: the vector unit)
        _lib.call("dicp_soft_match_backward", dev, dt, _p(x), _p(ctx.rx), n, _p(y), _p(ctx.ry), m, D, N, _p(v), C, ctx.tau, form, _p(out), _p(lse), _p(g),
                  _p(gx), _p(gy), _p(gv), _p(ws), need)
        return gx, gy, gv, None, None, None, None


def _check_temperature(temperature, fx, what):
    """a Python number > 0 whose scale -2 / temperature is a finite non-zero number of the tables' dtype -> float"""
    _number(temperature, what, "temperature must be a finite Python number > 0", 0.0, float("inf"), True, True)
    first = fx[0] if isinstance(fx, (list, tuple)) and fx else fx
    if isinstance(first, torch.Tensor) and first.dtype in _DT:
        c = torch.tensor(-2.0 / float(temperature), dtype=torch.float64).to(first.dtype)
        if not bool(torch.isfinite(c)) or float(c) == 0.0:
            raise ValueError("%s: -2 / temperature must be a finite non-zero %s, got temperature %r" % (what, first.dtype, temperature))
    return float(temperature)


def soft_match_features(fx, fy, values, temperature, x_rows=None, y_rows=None, return_best=False, _form=None):
    """Soft matches of two descriptor tables: for every row of fx the softmax-weighted mean of `values`, differentiable in fx, fy and values.

    fx, fy, x_rows, y_rows: as knn_features (a single table each, padded batches with optional row counts, or lists; float32 or float64;
        the same D in [1, 256]; CPU tensors are computed on the GPU and returned on the CPU).
    values: one row of C columns per row of fy, 1 <= C <= 8, in fy's form, dtype and device -- the target's xyz, or xyz + normal.
    temperature: a finite Python number tau > 0 (anything else is a ValueError before any device work).  A learnable temperature needs no
        gradient here: scaling both tables by tau^(-1/2) is the same operator at temperature 1.
    return_best: a bool; True also returns the hard winner and its probability.

    Definition (hardware-independent for every decision; T the dtype, fma and the channel order knn_features'):
        the score s_ij and the candidates of query i are knn_features', bit for bit (rows j < y_rows[b] with a finite score);
        c = (T)(-2.0 / tau), rounded once;  l_ij = c s_ij (one rounding);  p_ij = exp(l_ij - lse_i) over the candidates;
        out_i = sum_j p_ij values_j;  idx_i = the first candidate in (score, index) order = knn_features(k=1)'s, ties included;
        prob_i = p at idx_i.
    s_ij = (|x_i - y_j|^2 - |x_i|^2) / 2, so p is softmax_j(-|fx_i - fy_j|^2 / tau) exactly in exact arithmetic: the per-query constant
    cancels.  A query at or past x_rows[b], or without a candidate, gets a zero row, idx -1, prob 0 and exactly zero gradients whatever
    cotangent arrives; a row of fy at or past y_rows[b] enters no softmax and gets zero gradient whatever it and its values hold.  values
    are never examined: a non-finite value in a row below the count leaves that cloud's outputs unspecified (and nothing out of range).

    Returns out (n, C) / (N, n, C) / a list of (n_b, C); with return_best=True (out, idx, prob), idx int64 and prob in fx's dtype with
    one entry per row of fx.  idx and prob carry no gradient.

    The sums are an online softmax with a running maximum (|x|^2 / tau alone would overflow exp at small tau), in float32 with the scores
    on the matrix cores (v_mfma_f32_32x32x2_f32), in float64 on the vector unit; the (n, m) matrix is never formed.  The private _form
    ("valu" / "mfma") selects the float32 kernel for cross-checks: the two agree on idx exactly and on out to rounding (their orders of
    summation differ).

    float32 limit: the logits inherit the score's cancellation, an absolute error of about D u (|x||y| + |y|^2 / 2) 2 / tau with
    u = 2^-24.  For small tau normalise or centre the descriptors, or use float64.

    Gradients of out's cotangent g, with delta_i = g_i . out_i and a_ij = p_ij (g_i . values_j - delta_i):
        gfx_i = -c sum_j a_ij fy_j,   gfy_j = c (fy_j sum_i a_ij - sum_i a_ij fx_i),   gvalues_j = sum_i p_ij g_i.
    The backward recomputes the scores by the same chain and p from the saved lse; one pass owns the queries and one the rows of fy, every
    sum runs in a fixed order (float32 with D <= 128: scores and gradient products on the matrix cores, in the tiles' register order;
    otherwise the vector unit, in ascending index), every element is stored once: no atomics, no zero fill, the same bytes on every
    run.  Nothing is read back
    and every launch is on the current stream: a call on device tensors can sit in a captured graph, forward and backward.
    """
    what = "soft_match_features"
    tau = _check_temperature(temperature, fx, what)
    _flag(return_best, what, "return_best")
    code = _check_form(_form, fx, what)
    form, by, _, ylens = _clouds.check(fy, y_rows, what, "fy", "y_rows", empty_ok=True, min_cols=1)
    vform, bv, _, vlens = _clouds.check(values, None, what, "values", "y_rows", empty_ok=True, min_cols=1)
    if vform != form:
        raise ValueError("%s: values must have the form of fy (single tables, padded batches or lists), got %s and %s" % (what, vform, form))
    if bv.dtype != by.dtype or bv.device != by.device:
        raise ValueError("%s: values must have fy's dtype and device, got %s on %s" % (what, bv.dtype, bv.device))
    if not (1 <= bv.shape[2] <= C_MAX):
        raise ValueError("%s: values need C in [1, %d] columns, got %d" % (what, C_MAX, bv.shape[2]))
    if tuple(bv.shape[:2]) != tuple(by.shape[:2]) or vlens != ylens:
        raise ValueError("%s: values must hold one row per row of fy, got shape %s" % (what, tuple(bv.shape)))
    form, on_cpu, lens, n, m, xb, yb, rx, ry = _clouds.pair_features(fx, fy, x_rows, y_rows, what, D_MAX)
    _, vb, _ = _clouds.place(bv, None)
    out, idx, prob = _SoftMatch.apply(xb, yb, vb, rx, ry, tau, code)
    res = _clouds.restore(form, on_cpu, n, lens, [(ROW, out), (ROW, idx), (ROW, prob)])
    return res if return_best else res[0]


def _check_rules(mutual, ratio, max_d2, what):
    _flag(mutual, what, "mutual")
    _number(ratio, what, "ratio must be None or a number in (0, 1]", 0.0, 1.0, lo_open=True, none_ok=True)
    _number(max_d2, what, "max_d2 must be None or a number >= 0", 0.0, none_ok=True)


def match_features(fx, fy, x_rows=None, y_rows=None, mutual=True, ratio=None, max_d2=None, deterministic=False):
    """The accepted match in fy of every row of fx: nearest neighbour in descriptor space, mutual check, ratio test, distance gate.

    fx, fy, x_rows, y_rows, deterministic: as knn_features.
    ratio: None or a number in (0, 1] (Lowe's test on distances): the search takes k = 2, and a query is kept when d2_0 <= T(ratio ratio) d2_1;
        a query with a single candidate (d2_1 = +inf) passes.
    mutual: a bool; True runs the reverse k = 1 search (fy over fx, x_rows honoured) and keeps i when idx_yx[idx_xy[i]] == i.
    max_d2: None or a number >= 0: a query is kept when d2_0 <= max_d2.

    Returns (idx, d2): (n,) / (N, n) / lists of (n_b,); idx int64 -- the row of fy, -1 where the query is rejected or has no candidate --
    and d2 in fx's dtype, +inf where rejected.  d2 carries knn_features' gradient for the accepted rows; the decisions carry none, and a
    rejected row's gradient is exactly zero.  The rules read knn_features' outputs only; nothing is read back from the device.
    """
    _check_rules(mutual, ratio, max_d2, "match_features")
    _check_deterministic(deterministic, "match_features")
    form, on_cpu, lens, n, m, xb, yb, rx, ry = _clouds.pair_features(fx, fy, x_rows, y_rows, "match_features", D_MAX)
    d2k, idxk = _KnnFeatures.apply(xb, yb, rx, ry, 1 if ratio is None else 2, _lib.MATCH_AUTO, deterministic)
    d0, i0 = d2k[..., 0], idxk[..., 0]
    with torch.no_grad():
        keep = i0 >= 0
        if ratio is not None:
            r2 = torch.tensor(float(ratio) * float(ratio), dtype=d0.dtype, device=d0.device)
            keep &= d0 <= r2 * d2k[..., 1]
        if max_d2 is not None:
            keep &= d0 <= max_d2
        if mutual:
            _, back = _KnnFeatures.apply(yb.detach(), xb.detach(), ry, rx, 1, _lib.MATCH_AUTO, False)
            keep &= torch.gather(back[..., 0], 1, i0.clamp(min=0)) == torch.arange(xb.shape[1], device=i0.device)[None, :]
    idx = torch.where(keep, i0, torch.full_like(i0, -1))
    d2 = torch.where(keep, d0, torch.full_like(d0, float("inf")))
    return _clouds.restore(form, on_cpu, n, lens, [(ROW, idx), (ROW, d2)])
