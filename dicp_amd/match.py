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
"""
import torch

from . import _clouds, _lib
from ._clouds import ROW, K_MIN, K_MAX, _check_deterministic
from ._ops import _DT, _p
from .group import _invert

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
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not (0.0 < float(temperature) < float("inf")):
        raise ValueError("%s: temperature must be a finite Python number > 0, got %r" % (what, temperature))
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
    if not isinstance(return_best, bool):
        raise ValueError("%s: return_best must be True or False, got %r" % (what, return_best))
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
    if not isinstance(mutual, bool):
        raise ValueError("%s: mutual must be True or False, got %r" % (what, mutual))
    if ratio is not None and (isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not (0.0 < float(ratio) <= 1.0)):
        raise ValueError("%s: ratio must be None or a number in (0, 1], got %r" % (what, ratio))
    if max_d2 is not None and (isinstance(max_d2, bool) or not isinstance(max_d2, (int, float)) or not (float(max_d2) >= 0.0)):
        raise ValueError("%s: max_d2 must be None or a number >= 0, got %r" % (what, max_d2))


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
        T = torch.zeros((N, 4, 4), dtype=dt, device=dev)
        T[:, :3, :3] = pose[:, :9].reshape(N, 3, 3)
        T[:, :3, 3] = pose[:, 9:]
        T[:, 3, 3] = 1.0
        ctx.save_for_backward(x, y, w, idx, pose0, save)
        ctx.rows = rows
        return T

    @staticmethod
    def backward(ctx, gT):
        x, y, w, idx, pose0, save = ctx.saved_tensors
        N, n, _ = x.shape
        m = y.shape[1]
        dt, dev = x.dtype, x.device
        code = _DT[dt]
        gT = gT.contiguous()
        gpose = torch.cat((gT[:, :3, :3].reshape(N, 9), gT[:, :3, 3]), dim=1).contiguous()
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
    T = _align(xd, yd, idx_d, w, rows)
    if on_cpu:
        T = T.cpu()
    return T[0] if form == "single" else T


_NO_T = object()


def _pair_arguments(x, y, idx, weight, x_rows, what, T=_NO_T):
    """The checks of align_correspondences (and of a transform T, where one is given; ValueError before any device work), then its
    arguments on the device:
    -> (form, on_cpu, x (N,n,3), y (N,m,3), idx (N,n) as given, weight (N,n) or None, rows (N,) int32 or None)."""
    (form, bx, rx, _), (_, by, _, _) = _clouds.check_pair(x, y, x_rows, None, what)
    if form == "list":
        raise ValueError("%s: x and y must be single clouds or padded batches" % what)
    if bx.shape[1] < 1 or by.shape[1] < 1:
        raise ValueError("%s: x and y need at least one row" % what)
    N, n, m = bx.shape[0], bx.shape[1], by.shape[1]
    if not isinstance(idx, torch.Tensor) or idx.dtype not in (torch.int32, torch.int64):
        raise ValueError("%s: idx must be an int32 or int64 tensor, got %s" % (what, getattr(idx, "dtype", type(idx).__name__)))
    if tuple(idx.shape) != ((n,) if form == "single" else (N, n)) or idx.device != bx.device:
        raise ValueError("%s: idx must hold one entry per row of x on x's device, shape %s, got %s on %s"
                         % (what, (n,) if form == "single" else (N, n), tuple(idx.shape), idx.device))
    if not idx.is_cuda and idx.numel() and int(idx.max()) >= m:
        raise ValueError("%s: idx must be below y's %d rows" % (what, m))
    if weight is not None:
        if not isinstance(weight, torch.Tensor) or weight.dtype != bx.dtype or tuple(weight.shape) != tuple(idx.shape) or weight.device != bx.device:
            raise ValueError("%s: weight must be a tensor of x's dtype and device with idx's shape" % what)
    if T is not _NO_T:
        shape = (4, 4) if form == "single" else (N, 4, 4)
        if not isinstance(T, torch.Tensor) or T.dtype != bx.dtype or tuple(T.shape) != shape or T.device != bx.device:
            raise ValueError("%s: T must be a %s tensor of x's dtype on x's device" % (what, shape))
    on_cpu, xd, rows = _clouds.place(bx, rx, xyz=False)
    _, yd, _ = _clouds.place(by, None, xyz=False)
    dev = xd.device
    xd, yd = xd[..., :3].contiguous(), yd[..., :3].contiguous()
    idx_d = idx.to(dev).reshape(N, n)
    return form, on_cpu, xd, yd, idx_d, None if weight is None else weight.to(dev).reshape(N, n), rows


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


def _pose12(T):
    """(N, 4, 4) -> (N, 12): C row-major, then r"""
    return torch.cat((T[:, :3, :3].reshape(-1, 9), T[:, :3, 3]), dim=1).contiguous()


def _T44(pose):
    """(N, 12) -> (N, 4, 4)"""
    N = pose.shape[0]
    T = torch.zeros((N, 4, 4), dtype=pose.dtype, device=pose.device)
    T[:, :3, :3] = pose[:, :9].reshape(N, 3, 3)
    T[:, :3, 3] = pose[:, 9:]
    T[:, 3, 3] = 1.0
    return T


def _idx32(idx_d, m):
    """idx as the kernels read it: int32, anything at or past m clamped to m (the kernels clamp into [0, m - 1])"""
    return idx_d.clamp(min=-1, max=m).to(torch.int32).contiguous()


def _residuals(xd, yd, idx32, rows, pose):
    """dicp_pair_residuals on detached (N, n, 3) / (N, m, 3) points -> d2 (N, n)"""
    N, n, _ = xd.shape
    d2 = torch.empty((N, n), dtype=xd.dtype, device=xd.device)
    _lib.call("dicp_pair_residuals", xd.device, _DT[xd.dtype], _p(xd), _p(yd), _p(idx32), _p(rows), _p(pose), N, n, yd.shape[1], _p(d2))
    return d2


def _live_pairs(x0, y0, idx_d, rows):
    """Rule 1 of ransac_correspondences on detached (N, n, 3) / (N, m, 3) points -> (idx32 (N, n), live (N, n) bool, pairs (N, n, 6): every
    cloud's live rows (x[0:3], y[0:3]) packed first in ascending row order, P (N,) int32, index (N, n) int64: the row of every packed pair)"""
    from .filter import _Select
    N, n, _ = x0.shape
    m, dev = y0.shape[1], x0.device
    idx32 = _idx32(idx_d, m)
    yg = torch.gather(y0, 1, idx32.clamp(min=0, max=m - 1).long()[..., None].expand(N, n, 3))
    live = (idx32 >= 0) & torch.isfinite(x0).all(dim=-1) & torch.isfinite(yg).all(dim=-1)
    if rows is not None:
        live &= torch.arange(n, device=dev)[None, :] < rows[:, None]
    pairs, P, index = _Select.apply(torch.cat((x0, yg), dim=-1).contiguous(), live.contiguous(), None, True)
    return idx32, live, pairs, P, index


def _score_and_refine(x0, y0, idx_d, idx32, weight, rows, pairs, P, poses, threshold, refine, real=None):
    """The stages ransac_correspondences and consensus_correspondences share, from a cloud's hypothesis poses (N, H, 12) on (under
    torch.no_grad, on detached points): dicp_ransac_score, dicp_ransac_best, I_0 and the LO rounds -> (counts, best, best_count, pose_best,
    thr2, sets, accepted, round_poses, inliers).  real (N, H) bool: the hypotheses that exist; the counts of the others are zeroed before
    the choice."""
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
    minus = torch.full_like(idx_d, -1)
    for _ in range(int(refine)):
        pj = _pose12(_align(x0, y0, torch.where(inl, idx_d, minus), weight if weight is None else weight.detach(), rows))
        round_poses.append(pj)
        new = (_residuals(x0, y0, idx32, rows, pj) <= thr2) & some
        ok = new.sum(dim=1) >= inl.sum(dim=1)
        inl = torch.where(ok[:, None], new, inl)
        sets.append(inl)
        accepted.append(ok)
    return counts, best, best_count, pose_best, thr2, sets, accepted, round_poses, inl


def _ransac_stages(xd, yd, idx_d, weight, rows, threshold, hypotheses, seed, refine, _poses=None):
    """Every stage of ransac_correspondences on _pair_arguments' tensors, as a dict: live (N, n) bool, pairs (N, n, 6), P (N,) int32,
    index (N, n) int64, samples (N, H, 3) int32, poses (N, H, 12), counts (N, H) int32, best / best_count (N,) int32, pose_best (N, 12),
    thr2 (0-d), sets [I_0 .. I_R] of (N, n) bool, accepted [(N,) bool per round], round_poses [(N, 12) per round: T_j's pose], inliers (N, n)
    bool.  _poses (N, H, 12): the poses to
    score instead of stage 1's (samples are then -1).  Nothing is read back."""
    N, n, _ = xd.shape
    dt, dev = xd.dtype, xd.device
    code = _DT[dt]
    H = int(hypotheses)
    with torch.no_grad():
        x0, y0 = xd.detach(), yd.detach()
        idx32, live, pairs, P, index = _live_pairs(x0, y0, idx_d, rows)
        if _poses is None:
            poses = torch.empty((N, H, 12), dtype=dt, device=dev)
            samples = torch.empty((N, H, 3), dtype=torch.int32, device=dev)
            _lib.call("dicp_ransac_hypotheses", dev, code, _p(pairs), _p(P), N, n, H, int(seed) & 0xFFFFFFFF, _p(poses), _p(samples))
        else:
            poses = _poses.to(device=dev, dtype=dt).reshape(N, H, 12).contiguous()
            samples = torch.full((N, H, 3), -1, dtype=torch.int32, device=dev)
        counts, best, best_count, pose_best, thr2, sets, accepted, round_poses, inl = _score_and_refine(
            x0, y0, idx_d, idx32, weight, rows, pairs, P, poses, threshold, refine)
    return dict(live=live, pairs=pairs, P=P, index=index, samples=samples, poses=poses, counts=counts, best=best, best_count=best_count,
                pose_best=pose_best, thr2=thr2, sets=sets, accepted=accepted, round_poses=round_poses, inliers=inl)


def _check_ransac(threshold, hypotheses, seed, refine, return_hypothesis, what):
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not (0.0 < float(threshold) < float("inf")):
        raise ValueError("%s: threshold must be a finite number > 0, got %r" % (what, threshold))
    if isinstance(hypotheses, bool) or not isinstance(hypotheses, int) or not (1 <= hypotheses <= H_MAX):
        raise ValueError("%s: hypotheses must be an int in [1, %d], got %r" % (what, H_MAX, hypotheses))
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
        raise ValueError("%s: seed must be None or an int, got %r" % (what, seed))
    if isinstance(refine, bool) or not isinstance(refine, int) or not (0 <= refine <= REFINE_MAX):
        raise ValueError("%s: refine must be an int in [0, %d], got %r" % (what, REFINE_MAX, refine))
    if not isinstance(return_hypothesis, bool):
        raise ValueError("%s: return_hypothesis must be True or False, got %r" % (what, return_hypothesis))


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
    _check_ransac(threshold, hypotheses, seed, refine, return_hypothesis, what)
    form, on_cpu, xd, yd, idx_d, w, rows = _pair_arguments(x, y, idx, weight, x_rows, what)
    if seed is None:
        seed = int(torch.randint(0, 1 << 32, (1,), dtype=torch.int64).item())       # (a CPU tensor: no device read-back)
    st = _ransac_stages(xd, yd, idx_d, w, rows, threshold, hypotheses, seed, refine)
    inl = st["inliers"]
    T = _align(xd, yd, torch.where(inl, idx_d, torch.full_like(idx_d, -1)), w, rows)
    outs = [T, inl]
    if return_hypothesis:
        outs += [st["best"], st["best_count"], _T44(st["pose_best"])]
    if on_cpu:
        outs = [t.cpu() for t in outs]
    if form == "single":
        outs[0], outs[1] = outs[0][0], outs[1][0]
    return tuple(outs)


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
    if on_cpu:
        d2 = d2.cpu()
    return d2[0] if form == "single" else d2


GNC_ITER_MAX = 256      # GNC_ITER_MAX (csrc/dicp_gnc.h)
GNC_TRACE = 32          # GNC_TRACE: doubles of a trace record (mu, the band count, the 18 sums, the pose)
GNC_GROWTH_MAX = 16.0
GNC_LOSSES = {"tls": _lib.GNC_TLS, "gm": _lib.GNC_GM}


def _check_gnc(threshold, loss, growth, iterations, return_info, what):
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not (0.0 < float(threshold) < float("inf")) \
            or not (0.0 < float(threshold) * float(threshold) < float("inf")):
        raise ValueError("%s: threshold must be a finite number > 0 (with a finite square > 0), got %r" % (what, threshold))
    if not isinstance(loss, str) or loss not in GNC_LOSSES:
        raise ValueError('%s: loss must be "tls" or "gm", got %r' % (what, loss))
    if isinstance(growth, bool) or not isinstance(growth, (int, float)) or not (1.0 < float(growth) <= GNC_GROWTH_MAX):
        raise ValueError("%s: growth must be a finite number with 1 < growth <= %g, got %r" % (what, GNC_GROWTH_MAX, growth))
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not (1 <= iterations <= GNC_ITER_MAX):
        raise ValueError("%s: iterations must be an int in [1, %d], got %r" % (what, GNC_ITER_MAX, iterations))
    if not isinstance(return_info, bool):
        raise ValueError("%s: return_info must be True or False, got %r" % (what, return_info))


def _gnc_stages(xd, yd, idx_d, weight, rows, threshold, loss, growth, iterations, trace=False):
    """The kernel side of gnc_correspondences on _pair_arguments' tensors (under torch.no_grad, on detached points), as a dict: live
    (N, n) bool, pairs (N, n, 6), u (N, n) or None and P (N,) int32 (the packed pairs and their user weights), weights_packed (N, n),
    weights (N, n) in the original row order, rounds / status (N,) int32, mu (N,) float64, pose_last (N, 12), and with trace=True
    trace (N, iterations + 1, 32) float64, zero past a cloud's last record.  One dicp_gnc_fit launch; nothing is read back."""
    from .filter import _Select
    N, n, _ = xd.shape
    m, dt, dev = yd.shape[1], xd.dtype, xd.device
    with torch.no_grad():
        x0, y0 = xd.detach(), yd.detach()
        if weight is None:
            _, live, pairs, P, _ = _live_pairs(x0, y0, idx_d, rows)
            u = None
        else:                                                   # rule 1 with the weight's own condition; the weights ride along as a seventh column
            w0 = weight.detach()
            idx32 = _idx32(idx_d, m)
            yg = torch.gather(y0, 1, idx32.clamp(min=0, max=m - 1).long()[..., None].expand(N, n, 3))
            live = (idx32 >= 0) & torch.isfinite(x0).all(dim=-1) & torch.isfinite(yg).all(dim=-1) & torch.isfinite(w0) & (w0 > 0)
            if rows is not None:
                live &= torch.arange(n, device=dev)[None, :] < rows[:, None]
            packed, P, _ = _Select.apply(torch.cat((x0, yg, w0[..., None]), dim=-1).contiguous(), live.contiguous(), None, False)
            pairs, u = packed[..., :6].contiguous(), packed[..., 6].contiguous()
        wp = torch.empty((N, n), dtype=dt, device=dev)
        rounds = torch.empty((N,), dtype=torch.int32, device=dev)
        status = torch.empty((N,), dtype=torch.int32, device=dev)
        mu = torch.empty((N,), dtype=torch.float64, device=dev)
        pose = torch.empty((N, 12), dtype=dt, device=dev)
        tr = torch.zeros((N, int(iterations) + 1, GNC_TRACE), dtype=torch.float64, device=dev) if trace else None
        _lib.call("dicp_gnc_fit", dev, _DT[dt], _p(pairs), _p(P), _p(u), N, n, GNC_LOSSES[loss], float(threshold), float(growth), int(iterations),
                  _p(wp), _p(rounds), _p(status), _p(mu), _p(pose), _p(tr))
        pos = (torch.cumsum(live, dim=1) - 1).clamp(min=0)      # the packed position of every live row
        weights = torch.where(live, torch.gather(wp, 1, pos), torch.zeros((), dtype=dt, device=dev))
    return dict(live=live, pairs=pairs, u=u, P=P, weights_packed=wp, weights=weights, rounds=rounds, status=status, mu=mu, pose_last=pose, trace=tr)


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
    T = _align(xd, yd, torch.where(wg > 0, idx_d, torch.full_like(idx_d, -1)), wg if w is None else w * wg, rows)
    outs = [T, wg]
    if return_info:
        outs += [st["rounds"], st["status"], st["mu"], _T44(st["pose_last"])]
    if on_cpu:
        outs = [t.cpu() for t in outs]
    if form == "single":
        outs[0], outs[1] = outs[0][0], outs[1][0]
    return tuple(outs)


ITER_MAX = 64           # COMPAT_ITER_MAX (csrc/dicp_compat.h)


def _check_compat(threshold, iterations, min_length, what):
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not (0.0 < float(threshold) < float("inf")):
        raise ValueError("%s: threshold must be a finite number > 0, got %r" % (what, threshold))
    if isinstance(min_length, bool) or not isinstance(min_length, (int, float)) or not (0.0 <= float(min_length) < float("inf")):
        raise ValueError("%s: min_length must be a finite number >= 0, got %r" % (what, min_length))
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not (0 <= iterations <= ITER_MAX):
        raise ValueError("%s: iterations must be an int in [0, %d], got %r" % (what, ITER_MAX, iterations))


def _compat_stages(xd, yd, idx_d, rows, threshold, iterations, min_length, keep=None):
    """correspondence_compatibility (and, with keep, prune_correspondences) on _pair_arguments' tensors, as a dict: live (N, n) bool,
    pairs (N, n, 6), P (N,) int32, index (N, n) int64, score_packed (N, n) T and degree_packed (N, n) int32 (0 at and past P), score and
    degree in the original row order; with keep also rank_packed (N, n) int32, kept (N, n) bool and idx_kept.  Nothing is read back."""
    N, n, _ = xd.shape
    dt, dev = xd.dtype, xd.device
    code = _DT[dt]
    it = int(iterations)
    with torch.no_grad():
        idx32, live, pairs, P, index = _live_pairs(xd.detach(), yd.detach(), idx_d, rows)
        w = torch.empty((2, N, n), dtype=dt, device=dev)
        wmax = torch.zeros((max(it, 1), N), dtype=torch.int32 if dt == torch.float32 else torch.int64, device=dev)   # (the kernels take integer maxima)
        sp = torch.empty((N, n), dtype=dt, device=dev)
        dp = torch.empty((N, n), dtype=torch.int32, device=dev)
        _lib.call("dicp_compat_scores", dev, code, _p(pairs), _p(P), N, n, it, float(threshold), float(min_length), _p(w), _p(wmax), _p(sp), _p(dp))
        pos = (torch.cumsum(live, dim=1) - 1).clamp(min=0)                  # the packed position of every live row
        score = torch.where(live, torch.gather(sp, 1, pos), torch.zeros((), dtype=dt, device=dev))
        degree = torch.where(live, torch.gather(dp, 1, pos), torch.zeros((), dtype=torch.int32, device=dev))
        st = dict(live=live, pairs=pairs, P=P, index=index, score_packed=sp, degree_packed=dp, score=score, degree=degree)
        if keep is not None:
            rank = torch.empty((N, n), dtype=torch.int32, device=dev)
            _lib.call("dicp_compat_rank", dev, code, _p(sp), _p(P), N, n, _p(rank))
            kept = live & (torch.gather(rank, 1, pos) < min(int(keep), 0x7fffffff))
            st.update(rank_packed=rank, kept=kept, idx_kept=torch.where(kept, idx_d, torch.full_like(idx_d, -1)))
    return st


def _compat_outputs(form, on_cpu, outs):
    if on_cpu:
        outs = [t.cpu() for t in outs]
    return tuple(t[0] if form == "single" else t for t in outs)


def correspondence_compatibility(x, y, idx, threshold, iterations=10, min_length=0.0, x_rows=None):
    """The spatial-compatibility score and degree of every correspondence: which matches keep their lengths to each other, as all correct
    matches do under a rigid motion and wrong ones only by accident (spectral matching; the first-order compatibility of SC2-PCR / PointDSC).

    x, y, idx, x_rows: exactly as align_correspondences / ransac_correspondences (single clouds or padded batches, float32 or float64,
        columns 0:3, idx int32 or int64 with negative = no match; CPU tensors are computed on the GPU and returned on the CPU).
    threshold: a finite number > 0, the largest change of a length.  min_length: a finite number >= 0.  iterations: an int in [0, 64].
    Anything else is a ValueError before any device work.

    Definition (hardware-independent; T the points' dtype, fma its correctly rounded fused multiply-add, sqrt and / correctly rounded):
     1. The live pairs are those of rule 1 of ransac_correspondences, packed in ascending row order: P per cloud, (x_p, y_p) each.
     2. Packed positions p != q are compatible iff |e| <= thr and a >= L and b >= L, thr = T(threshold), L = T(min_length), where
            A = +0, A = fma(t_a, t_a, A) for a = 0, 1, 2 with t_a = x_pa - x_qa;  B likewise from y;  a = sqrt(A), b = sqrt(B), e = a - b.
        Every comparison with a NaN is false.  The relation is symmetric bit for bit.  With min_length > 0, matches that share a source or a
        target point stop vouching for each other.
     3. degree_p = the number of q != p below P compatible with p.
     4. v^0 = 1.  For t = 1 .. iterations: w_p = the sum over q = 0 .. P - 1 in ascending q of v^{t-1}_q over the q compatible with p or equal
        to p (the matrix M + I: the same eigenvectors, no oscillation), added sequentially in T from +0, one rounding per addition;
        wmax = max_p w_p (>= 1 whenever P >= 1);  v^t_p = w_p / wmax.  score = v^iterations: the power iteration towards the leading
        eigenvector, normalised to a maximum of 1.  w^1 = degree + 1 exactly for P < 2^24; iterations = 0 gives score 1 on the live rows.

    Returns (score, degree): (N, n) or (n,), score in x's dtype and degree int32, in the original row order, 0 on rows that are not live.
    Neither requires grad: they are decisions.  Nothing is read back and no launch shape depends on device data: a call on device tensors
    can sit in a captured graph.  No float atomics: the same bytes on every run.

    Kernels (libdicp_hip.so): dicp_select_rows packs the live pairs; dicp_compat_scores runs one pass over all P^2 pairs per iteration, a
    lane per row p walking q in LDS tiles, O(n) memory per cloud.
    """
    what = "correspondence_compatibility"
    _check_compat(threshold, iterations, min_length, what)
    form, on_cpu, xd, yd, idx_d, _, rows = _pair_arguments(x, y, idx, None, x_rows, what)
    st = _compat_stages(xd, yd, idx_d, rows, threshold, iterations, min_length)
    return _compat_outputs(form, on_cpu, [st["score"], st["degree"]])


def prune_correspondences(x, y, idx, threshold, keep, iterations=10, min_length=0.0, x_rows=None, order=1):
    """The `keep` most compatible correspondences of every cloud: the step between match_features and ransac_correspondences when most of
    the matches are wrong.

    x, y, idx, threshold, iterations, min_length, x_rows: as correspondence_compatibility.  keep: an int >= 1; order: 1 or 2 (anything else
    is a ValueError before any device work).

     5. With score of correspondence_compatibility, the rank of live pair p is the number of live q with score_q > score_p, or
        score_q == score_p and q < p; a pair is kept iff its rank < keep.  keep >= P keeps every live pair.

    order=2 ranks by the second-order degree instead (rules 6-8 of second_order_compatibility: a pair is kept iff rank2 < keep), ignores
    `iterations` and returns score2 as score: one pass that separates better than the ten first-order passes when the inliers are few,
    at O(n^2 / 8) bytes per cloud.

    Returns (idx_kept, score): idx_kept has idx's dtype and shape, idx where the row is kept and -1 elsewhere -- it feeds
    align_correspondences / ransac_correspondences / correspondence_residuals unchanged; score as correspondence_compatibility's.  No
    gradient, nothing read back, bit-reproducible, fit for a captured graph.  Kernels: those of correspondence_compatibility and
    dicp_compat_rank, a second, much cheaper pass over the P^2 pairs; order=2: those of second_order_compatibility.
    """
    what = "prune_correspondences"
    _check_compat(threshold, iterations, min_length, what)
    if isinstance(keep, bool) or not isinstance(keep, int) or keep < 1:
        raise ValueError("%s: keep must be an int >= 1, got %r" % (what, keep))
    if isinstance(order, bool) or order not in (1, 2):
        raise ValueError("%s: order must be 1 or 2, got %r" % (what, order))
    form, on_cpu, xd, yd, idx_d, _, rows = _pair_arguments(x, y, idx, None, x_rows, what)
    if order == 2:
        st = _compat2_stages(xd, yd, idx_d, rows, threshold, min_length, keep=keep)
        return _compat_outputs(form, on_cpu, [st["idx_kept"], st["score2"]])
    st = _compat_stages(xd, yd, idx_d, rows, threshold, iterations, min_length, keep=keep)
    return _compat_outputs(form, on_cpu, [st["idx_kept"], st["score"]])


N2_MAX = 1 << 20        # COMPAT2_N_MAX (csrc/dicp_compat2.h)
MEMBERS_MIN, MEMBERS_MAX = 3, 32


def _compat2_stages(xd, yd, idx_d, rows, threshold, min_length, keep=None, seeds=None, members=None):
    """second_order_compatibility (with keep, prune_correspondences(order=2); with seeds and members, the hypotheses of
    consensus_correspondences) on _pair_arguments' tensors, as a dict: idx32, live (N, n) bool, pairs (N, n, 6), P (N,) int32, index,
    adj (N, n, W) int64, degree_packed (N, n) int32, degree2_packed (N, n) int64, rank2_packed (N, n) int32, score2_packed (N, n) T, and
    score2 / degree2 / degree in the original row order; with keep also kept and idx_kept; with seeds also seedpos (N, seeds) int32 (only
    the entries below min(seeds, P) are written), members (N, seeds, members) int32, poses (N, seeds, 12) T and real (N, seeds) bool.
    Nothing is read back."""
    N, n, _ = xd.shape
    dt, dev = xd.dtype, xd.device
    code = _DT[dt]
    if n > N2_MAX or N * n * ((n + 63) // 64) >= 1 << 40:
        raise ValueError("second-order compatibility: %d clouds of %d rows need %d bytes of adjacency bits: too many" % (N, n, N * n * ((n + 63) // 64) * 8))
    W = (n + 63) // 64
    H = 0 if seeds is None else int(seeds)
    with torch.no_grad():
        idx32, live, pairs, P, index = _live_pairs(xd.detach(), yd.detach(), idx_d, rows)
        adj = torch.empty((N, n, W), dtype=torch.int64, device=dev)
        dp = torch.empty((N, n), dtype=torch.int32, device=dev)
        d2p = torch.empty((N, n), dtype=torch.int64, device=dev)
        rank = torch.empty((N, n), dtype=torch.int32, device=dev)
        s2p = torch.empty((N, n), dtype=dt, device=dev)
        seedpos = torch.empty((N, H), dtype=torch.int32, device=dev) if H else None
        _lib.call("dicp_compat2_bits", dev, code, _p(pairs), _p(P), N, n, float(threshold), float(min_length), _p(adj), _p(dp), _p(d2p))
        _lib.call("dicp_compat2_common", dev, _p(adj), _p(P), N, n, _p(d2p))
        _lib.call("dicp_compat2_rank", dev, code, _p(d2p), _p(P), N, n, H, _p(rank), _p(s2p), _p(seedpos))
        pos = (torch.cumsum(live, dim=1) - 1).clamp(min=0)                  # the packed position of every live row
        score2 = torch.where(live, torch.gather(s2p, 1, pos), torch.zeros((), dtype=dt, device=dev))
        degree2 = torch.where(live, torch.gather(d2p, 1, pos), torch.zeros((), dtype=torch.int64, device=dev))
        degree = torch.where(live, torch.gather(dp, 1, pos), torch.zeros((), dtype=torch.int32, device=dev))
        st = dict(idx32=idx32, live=live, pairs=pairs, P=P, index=index, adj=adj, degree_packed=dp, degree2_packed=d2p, rank2_packed=rank,
                  score2_packed=s2p, score2=score2, degree2=degree2, degree=degree)
        if keep is not None:
            kept = live & (torch.gather(rank, 1, pos) < min(int(keep), 0x7fffffff))
            st.update(kept=kept, idx_kept=torch.where(kept, idx_d, torch.full_like(idx_d, -1)))
        if H:
            K = int(members)
            mem = torch.empty((N, H, K), dtype=torch.int32, device=dev)
            poses = torch.empty((N, H, 12), dtype=dt, device=dev)
            _lib.call("dicp_compat2_seeds", dev, code, _p(pairs), _p(P), _p(adj), _p(seedpos), N, n, H, K, _p(mem), _p(poses))
            st.update(seedpos=seedpos, members=mem, poses=poses, real=mem[:, :, 2] >= 0)
    return st


def _check_compat2(threshold, min_length, what):
    _check_compat(threshold, 0, min_length, what)


def second_order_compatibility(x, y, idx, threshold, min_length=0.0, x_rows=None, return_adjacency=False):
    """The second-order spatial compatibility (SC2) of every correspondence: how many triangles of mutually compatible matches pass
    through it.  Two correct matches share every other correct match as a common compatible neighbour; a wrong match compatible with a
    correct one by accident shares almost none -- so the measure separates a handful of inliers from accidental degrees that the
    first-order degree of correspondence_compatibility cannot tell apart.

    x, y, idx, threshold, min_length, x_rows: exactly as correspondence_compatibility.  return_adjacency: a bool.

    Definition (continues rules 1-5 of correspondence_compatibility; integers only from rule 6 on):
     6. W = ceil(n / 64).  adj (N, n, W) int64 over the PACKED positions: bit q % 64 of word q // 64 of row p, counted from the least
        significant bit, is 1 iff p < P, q < P, p != q and p, q are compatible by rule 2; every other bit is 0.
     7. common(p, q) = sum_w popcount(adj[p, w] & adj[q, w]);  S(p, q) = common(p, q) if bit (p, q) is set, else 0 (the matrix M o M^2);
        degree2_p = sum_q S(p, q), an int64: twice the triangles through p.
     8. rank2_p = the number of live q with degree2_q > degree2_p, or degree2_q == degree2_p and q < p, compared as integers.
        score2_p = T(degree2_p) / T(max_q degree2_q), both operations correctly rounded; 0 where the maximum is 0.

    Returns (score2, degree2, degree): (N, n) or (n,) in the original row order -- score2 in x's dtype, degree2 int64, degree int32 (rule 3)
    -- 0 on rows that are not live; with return_adjacency=True also adj (N, n, W) / (n, W) int64, in packed order.  No gradient.

    Memory: N n W 8 bytes of adjacency bits, O(n^2 / 8) per cloud -- 32 MB per cloud at n = 16384; shapes with n > 2^20 or 2^40 words and
    more are a ValueError.  Time: n^2 W word pairs per cloud: faster than ten first-order passes at a few thousand matches, slower from
    about ten thousand on (README, "Second-order compatibility").  A clique of wrong matches that keep their lengths to each other by
    accident can outrank the inliers when it is as large as their set.

    Nothing is read back, the grids are sized by n, and no launch depends on device data: a call on device tensors can sit in a captured
    graph.  The only atomics are integer additions: the same bytes on every run.

    Kernels (libdicp_hip.so): dicp_select_rows packs the live pairs; dicp_compat2_bits (one first-order pass that stores its decisions as
    bits), dicp_compat2_common (AND + popcount over the rows' words, a register tile of counts per lane), dicp_compat2_rank.
    """
    what = "second_order_compatibility"
    _check_compat2(threshold, min_length, what)
    if not isinstance(return_adjacency, bool):
        raise ValueError("%s: return_adjacency must be True or False, got %r" % (what, return_adjacency))
    form, on_cpu, xd, yd, idx_d, _, rows = _pair_arguments(x, y, idx, None, x_rows, what)
    st = _compat2_stages(xd, yd, idx_d, rows, threshold, min_length)
    outs = [st["score2"], st["degree2"], st["degree"]]
    if return_adjacency:
        outs.append(st["adj"])
    return _compat_outputs(form, on_cpu, outs)


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
    _check_compat2(threshold, min_length, what)
    thr_in = threshold if inlier_threshold is None else inlier_threshold
    if isinstance(seeds, bool) or not isinstance(seeds, int) or not (1 <= seeds <= H_MAX):
        raise ValueError("%s: seeds must be an int in [1, %d], got %r" % (what, H_MAX, seeds))
    if isinstance(thr_in, bool) or not isinstance(thr_in, (int, float)) or not (0.0 < float(thr_in) < float("inf")):
        raise ValueError("%s: inlier_threshold must be None or a finite number > 0, got %r" % (what, inlier_threshold))
    _check_ransac(thr_in, seeds, None, refine, return_hypothesis, what)
    if isinstance(members, bool) or not isinstance(members, int) or not (MEMBERS_MIN <= members <= MEMBERS_MAX):
        raise ValueError("%s: members must be an int in [%d, %d], got %r" % (what, MEMBERS_MIN, MEMBERS_MAX, members))
    form, on_cpu, xd, yd, idx_d, w, rows = _pair_arguments(x, y, idx, weight, x_rows, what)
    st = _consensus_stages(xd, yd, idx_d, w, rows, threshold, thr_in, seeds, members, refine, min_length)
    inl = st["inliers"]
    T = _align(xd, yd, torch.where(inl, idx_d, torch.full_like(idx_d, -1)), w, rows)
    outs = [T, inl]
    if return_hypothesis:
        outs += [st["best"], st["best_count"], _T44(st["pose_best"]), st["members"]]
    if on_cpu:
        outs = [t.cpu() for t in outs]
    if form == "single":
        outs[0], outs[1] = outs[0][0], outs[1][0]
    return tuple(outs)


def _consensus_stages(xd, yd, idx_d, weight, rows, threshold, inlier_threshold, seeds, members, refine, min_length):
    """Every stage of consensus_correspondences on _pair_arguments' tensors: _compat2_stages' dict plus _score_and_refine's outputs under
    the names _ransac_stages uses.  Nothing is read back."""
    st = _compat2_stages(xd, yd, idx_d, rows, threshold, min_length, seeds=seeds, members=members)
    with torch.no_grad():
        counts, best, best_count, pose_best, thr2, sets, accepted, round_poses, inl = _score_and_refine(
            xd.detach(), yd.detach(), idx_d, st["idx32"], weight, rows, st["pairs"], st["P"], st["poses"], inlier_threshold, refine, real=st["real"])
    st.update(counts=counts, best=best, best_count=best_count, pose_best=pose_best, thr2=thr2, sets=sets, accepted=accepted, round_poses=round_poses,
              inliers=inl)
    return st
