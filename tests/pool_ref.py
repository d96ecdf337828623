"""The definition of dicp_amd.group.pool_neighbors in numpy, for one cloud: a feature table f (m, C), indices idx (n, k), optionally rows.

pool_ref restates the docstring with one numpy operation per rounding, in the table's dtype T, looping over the k slots in slot order;
pool_exact evaluates the sum and the mean in float64 on the same inputs and returns the sum of magnitudes that the mean's bound is made
of.  The makers below build the tables that put ties and NaNs where the maximum's rules differ from one another.  Built on group_ref's
live_slots / make_idx.  A plain module (no fixtures): the tests put this directory on sys.path and import it.
"""
import numpy as np

import group_ref as gr

REDUCES = ("sum", "mean", "max")


def pool_ref(f, idx, reduce, rows=None, tie=">", lose_slot=False, nan_propagates=True, argmax_row=True):
    """-> out (n, C) in f's dtype, argmax (n, C) int32 (the winning slot's ROW; -1 without a live slot; all -1 for sum / mean),
    counts (n,) int32.

    The keywords make the deliberately wrong restatements that the tests show the comparison to refuse: tie=">=" lets a later equal value
    win, lose_slot skips each query's last live slot, nan_propagates=False leaves NaNs out of the comparison (they lose every one),
    argmax_row=False reports the slot number."""
    T = f.dtype.type
    n, k = idx.shape
    C = f.shape[1]
    live = gr.live_slots(idx, f.shape[0], rows)
    counts = live.sum(1).astype(np.int32)
    if lose_slot:
        last = k - 1 - live[:, ::-1].argmax(1)
        live = live.copy()
        live[np.arange(n), last] = False
    x = f[np.where(live, idx, 0)]                            # (n, k, C); empty slots read row 0 and are masked below
    acc = np.zeros((n, C), dtype=T)
    arg = np.full((n, C), -1, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(k):
            on = live[:, s, None]
            v = x[:, s]
            if reduce == "max":
                first = arg < 0
                better = (v >= acc) if tie == ">=" else (v > acc)
                if nan_propagates:
                    better = better | (np.isnan(v) & ~np.isnan(acc))
                take = on & (first | better)
                acc = np.where(take, v, acc)
                arg = np.where(take, (idx[:, s, None] if argmax_row else s), arg)
            else:
                acc = np.where(on, (acc + v).astype(T), acc)
        if reduce == "mean":
            cnt = live.sum(1)
            acc = np.where(cnt[:, None] > 0, (acc / np.maximum(cnt, 1).astype(T)[:, None]).astype(T), T(0)).astype(T)
    return acc.astype(T), arg.astype(np.int32), counts


def pool_exact(f, idx, reduce, rows=None):
    """float64 on the same inputs -> (the sum or the mean (n, C), sum_s |f[idx_s, c]| (n, C) over the live slots, counts (n,))"""
    live = gr.live_slots(idx, f.shape[0], rows)
    x = np.where(live[:, :, None], f.astype(np.float64)[np.where(live, idx, 0)], 0.0)
    cnt = live.sum(1)
    val = x.sum(1)
    if reduce == "mean":
        val = val / np.maximum(cnt, 1)[:, None]
    return val, np.abs(x).sum(1), cnt


def mean_bound(k, dtype):
    """the factor of sum|f| / count in the mean's bound: (k + 2) u -- k - 1 additions at u each and a division allowed one ulp, rounded up"""
    return (k + 2) * float(np.finfo(dtype).eps) / 2


def mean_ratio(got, f, idx, rows=None):
    """the largest |got - exact mean| / bound over the queries with a live slot; entries whose bound is 0 must be exact"""
    ex, mag, cnt = pool_exact(f, idx, "mean", rows)
    k = idx.shape[1]
    bound = mean_bound(k, f.dtype) * mag / np.maximum(cnt, 1)[:, None]
    err = np.abs(got.astype(np.float64) - ex)
    assert (err[bound == 0] == 0).all()
    on = bound > 0
    return float((err[on] / bound[on]).max()) if on.any() else 0.0


def same_result(got, want, nan_ok=False):
    """(out, argmax, counts) against (out, argmax, counts): dtypes, shapes and bits.  nan_ok: NaNs of the output compare equal whatever
    their sign and payload (an inf - inf made by an ADDITION has the adder's NaN, not a table value's)"""
    go, ga, gc = got
    wo, wa, wc = want
    if go.dtype != wo.dtype or go.shape != wo.shape:
        return False
    if nan_ok:
        both = np.isnan(go) & np.isnan(wo)
        go, wo = np.where(both, 0, go), np.where(both, 0, wo)
    ok = gr.same_bits(np.ascontiguousarray(go), np.ascontiguousarray(wo))
    if ga is not None:
        ok = ok and ga.dtype == np.int32 and np.array_equal(ga, wa)
    if gc is not None:
        ok = ok and gc.dtype == np.int32 and np.array_equal(gc, wc)
    return bool(ok)


# ------------------------------------------------------------------ test inputs
TIE_VALUES = (-2.0, -1.0, -0.0, 0.0, 1.0, 2.0, np.inf, -np.inf)


def make_tie_table(m, C, dtype, seed):
    """(m, C) drawn from eight values, +0 / -0 and +-inf among them: with k = 8 slots most queries hold their maximum more than once"""
    rng = np.random.default_rng(seed)
    return np.array(TIE_VALUES, dtype=dtype)[rng.integers(0, len(TIE_VALUES), size=(m, C))]


def tie_kinds(f, idx, rows=None):
    """what the tie table promises: queries whose MAXIMUM is held by several live slots naming different rows, and queries where the tie
    at the top is between +0 and -0"""
    live = gr.live_slots(idx, f.shape[0], rows)
    x = f[np.where(live, idx, 0)].astype(np.float64)
    x = np.where(live[:, :, None], x, -np.inf)
    top = x.max(1, keepdims=True)
    at_top = (x == top) & live[:, :, None]
    rows_at = np.where(at_top, idx[:, :, None], -1)
    several = (at_top.sum(1) >= 2) & (rows_at.max(1) != np.where(at_top, idx[:, :, None], 2 ** 62).min(1))
    sign = np.signbit(f[np.where(live, idx, 0)])
    zeros = (top[:, 0] == 0) & (at_top & sign).any(1) & (at_top & ~sign).any(1)
    return {"tied_maximum": int(several.sum()), "signed_zero_tie": int(zeros.sum()), "queries": int(live.any(1).sum())}


def make_nan_case(n, k, m, C, dtype, seed):
    """-> f (m, C), idx (n, k), where (n,) in {-1: no NaN, 0: first, 1: a middle, 2: the last live slot}: queries i % 4 in {1, 2, 3} with at
    least three live slots read a row of NaNs (rows m - 3 .. m - 1, named nowhere else) in that position; some of them a second NaN row
    later on, which must not take the argmax over"""
    rng = np.random.default_rng(seed)
    f = ((rng.random((m, C)) * 2 - 1) * 10.0 ** rng.integers(-2, 3, size=(m, C))).astype(dtype)
    f[m - 3:] = np.nan
    idx = gr.make_idx(n, k, m - 3, m - 3, seed + 1)
    idx = np.where((idx >= m - 3) & (idx < m), -1, idx)      # (make_idx's "exactly rows" slots would name the NaN rows)
    where = np.full(n, -1)
    live = gr.live_slots(idx, m, m)
    for i in range(n):
        ls = np.flatnonzero(live[i])
        if i % 4 == 0 or len(ls) < 3:
            continue
        pos = i % 4 - 1
        s = (ls[0], ls[len(ls) // 2], ls[-1])[pos]
        idx[i, s] = m - 3 + pos
        where[i] = pos
        if pos == 0 and i % 8 == 1:
            idx[i, ls[-1]] = m - 1                           # a second NaN, another row: the first one keeps the argmax
    return f, idx, where
