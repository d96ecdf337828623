"""Pruning of explicit correspondences by spatial compatibility, first order (the power iteration of spectral matching) and second
order (SC2: triangles of compatible matches, on packed adjacency bits).  match.py holds the overview of the whole chain and re-exports
every public name here; register.py builds consensus_correspondences on _compat2_stages.
"""
import torch

from . import _lib
from ._ops import _DT, _p
from ._pairs import _finish, _flag, _int_in, _live_pairs, _number, _pair_arguments, _threshold

ITER_MAX = 64           # COMPAT_ITER_MAX (csrc/dicp_compat.h)


def _check_compat(threshold, iterations, min_length, what):
    _threshold(threshold, what)
    _number(min_length, what, "min_length must be a finite number >= 0", 0.0, float("inf"), hi_open=True)
    _int_in(iterations, what, "iterations", 0, ITER_MAX)


def _compat_stages(xd, yd, idx_d, rows, threshold, iterations, min_length, keep=None):
    """correspondence_compatibility (and, with keep, prune_correspondences) on _pair_arguments' tensors, as a dict: live (N, n) bool,
    pairs (N, n, 6), P (N,) int32, index (N, n) int64, score_packed (N, n) T and degree_packed (N, n) int32 (0 at and past P), score and
    degree in the original row order; with keep also rank_packed (N, n) int32, kept (N, n) bool and idx_kept.  Nothing is read back."""
    N, n, _ = xd.shape
    dt, dev = xd.dtype, xd.device
    code = _DT[dt]
    it = int(iterations)
    with torch.no_grad():
        pk = _live_pairs(xd.detach(), yd.detach(), idx_d, rows)
        w = torch.empty((2, N, n), dtype=dt, device=dev)
        wmax = torch.zeros((max(it, 1), N), dtype=torch.int32 if dt == torch.float32 else torch.int64, device=dev)   # (the kernels take integer maxima)
        sp = torch.empty((N, n), dtype=dt, device=dev)
        dp = torch.empty((N, n), dtype=torch.int32, device=dev)
        _lib.call("dicp_compat_scores", dev, code, _p(pk.pairs), _p(pk.P), N, n, it, float(threshold), float(min_length), _p(w), _p(wmax), _p(sp), _p(dp))
        st = dict(live=pk.live, pairs=pk.pairs, P=pk.P, index=pk.index, score_packed=sp, degree_packed=dp, score=pk.unpack(sp), degree=pk.unpack(dp))
        if keep is not None:
            rank = torch.empty((N, n), dtype=torch.int32, device=dev)
            _lib.call("dicp_compat_rank", dev, code, _p(sp), _p(pk.P), N, n, _p(rank))
            kept, idx_kept = pk.keep(rank, keep, idx_d)
            st.update(rank_packed=rank, kept=kept, idx_kept=idx_kept)
    return st


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
    return _finish(form, on_cpu, [st["score"], st["degree"]], 2)


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
    _number(keep, what, "keep must be an int >= 1", 1, integer=True)
    if isinstance(order, bool) or order not in (1, 2):
        raise ValueError("%s: order must be 1 or 2, got %r" % (what, order))
    form, on_cpu, xd, yd, idx_d, _, rows = _pair_arguments(x, y, idx, None, x_rows, what)
    if order == 2:
        st = _compat2_stages(xd, yd, idx_d, rows, threshold, min_length, keep=keep)
        return _finish(form, on_cpu, [st["idx_kept"], st["score2"]], 2)
    st = _compat_stages(xd, yd, idx_d, rows, threshold, iterations, min_length, keep=keep)
    return _finish(form, on_cpu, [st["idx_kept"], st["score"]], 2)


N2_MAX = 1 << 20        # COMPAT2_N_MAX (csrc/dicp_compat2.h)


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
        pk = _live_pairs(xd.detach(), yd.detach(), idx_d, rows)
        pairs, P = pk.pairs, pk.P
        adj = torch.empty((N, n, W), dtype=torch.int64, device=dev)
        dp = torch.empty((N, n), dtype=torch.int32, device=dev)
        d2p = torch.empty((N, n), dtype=torch.int64, device=dev)
        rank = torch.empty((N, n), dtype=torch.int32, device=dev)
        s2p = torch.empty((N, n), dtype=dt, device=dev)
        seedpos = torch.empty((N, H), dtype=torch.int32, device=dev) if H else None
        _lib.call("dicp_compat2_bits", dev, code, _p(pairs), _p(P), N, n, float(threshold), float(min_length), _p(adj), _p(dp), _p(d2p))
        _lib.call("dicp_compat2_common", dev, _p(adj), _p(P), N, n, _p(d2p))
        _lib.call("dicp_compat2_rank", dev, code, _p(d2p), _p(P), N, n, H, _p(rank), _p(s2p), _p(seedpos))
        st = dict(idx32=pk.idx32, live=pk.live, pairs=pairs, P=P, index=pk.index, adj=adj, degree_packed=dp, degree2_packed=d2p, rank2_packed=rank,
                  score2_packed=s2p, score2=pk.unpack(s2p), degree2=pk.unpack(d2p), degree=pk.unpack(dp))
        if keep is not None:
            st["kept"], st["idx_kept"] = pk.keep(rank, keep, idx_d)
        if H:
            K = int(members)
            mem = torch.empty((N, H, K), dtype=torch.int32, device=dev)
            poses = torch.empty((N, H, 12), dtype=dt, device=dev)
            _lib.call("dicp_compat2_seeds", dev, code, _p(pairs), _p(P), _p(adj), _p(seedpos), N, n, H, K, _p(mem), _p(poses))
            st.update(seedpos=seedpos, members=mem, poses=poses, real=mem[:, :, 2] >= 0)
    return st


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
    _check_compat(threshold, 0, min_length, what)
    _flag(return_adjacency, what, "return_adjacency")
    form, on_cpu, xd, yd, idx_d, _, rows = _pair_arguments(x, y, idx, None, x_rows, what)
    st = _compat2_stages(xd, yd, idx_d, rows, threshold, min_length)
    outs = [st["score2"], st["degree2"], st["degree"]]
    if return_adjacency:
        outs.append(st["adj"])
    return _finish(form, on_cpu, outs, len(outs))
