"""The definition of the deterministic y-gradient of knn_points / ball_query / chamfer_distance (deterministic=True) in numpy, for one cloud.

knn_det_ref restates dicp_amd/csrc/dicp_knn_det.h: per row l < rows of y the walk over the row's list in the inverted index of idx
(inverse_ref.invert_ref's, with the walk's clamps and its entry check), the term of each entry, and inverse_ref.chunked_sum's order of
summation -- one numpy operation per rounding.  The `wrong` keyword makes the deliberately wrong restatements that the tests show the
comparison to refuse.  knn_det_bound derives how far the rule may lie from the exact sum.  A plain module (no fixtures): the tests put this
directory on sys.path and import it.
"""
import numpy as np

import inverse_ref as ir
import walk_layouts as wl
from dicp_amd.group import DET_CHUNK

WRONG = ("descending", "lose_entry", "sum_wide", "no_zero_skip", "chunk_off_by_one")


def chunked_sum_fast(terms, has, D=DET_CHUNK):
    """inverse_ref.chunked_sum for `has` constant along a row, a chunk at a time: numpy's accumulate adds sequentially, one rounding per
    addition, from a +0 put in front.  Held to chunked_sum bit for bit on every input of tests/test_knn_det_host.py; the GPU tests use
    it on the long lists."""
    T = terms.dtype.type
    L, C = terms.shape
    total, part = np.zeros(C, dtype=T), np.zeros(C, dtype=T)
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, max(L, 1), D):
            if c0 > 0:
                total = (total + part).astype(T)
            sel = terms[c0:c0 + D][has[c0:c0 + D, 0]]
            part = np.add.accumulate(np.concatenate([np.zeros((1, C), dtype=T), sel]), axis=0, dtype=T)[-1]
        return part if L <= D else (total + part).astype(T)


def knn_det_ref(g, idx, x, y, rows, offsets, slots, D=DET_CHUNK, wrong=None, fast=False):
    """g (n, k) in dtype T, idx (n, k) integer, x (n, cx) and y (m, cy) in T, rows: the live rows of y (None: m), offsets (m + 1,) and
    slots (n k,) the inverted index -> (m, cy) in T.

    wrong: "descending" walks each list backwards; "lose_entry" drops the last entry of a list; "sum_wide" sums the unrounded terms in
    a wider type (float64 for float32, long double for float64) and rounds at the end; "no_zero_skip" gives an entry with g = 0 its
    term (0 * inf = NaN behind an inf coordinate); "chunk_off_by_one" starts every chunk one position early.  fast: chunked_sum_fast."""
    csum = chunked_sum_fast if fast else ir.chunked_sum
    T = g.dtype.type
    n, k = idx.shape
    nk, m, cy = n * k, y.shape[0], y.shape[1]
    lim = m if rows is None else min(max(int(rows), 0), m)
    row = ir.slot_rows(idx, m, rows).reshape(-1)
    gf = g.reshape(-1)
    wide = np.float64 if T == np.float32 else np.longdouble
    out = np.zeros((m, cy), dtype=T)
    with np.errstate(invalid="ignore", over="ignore"):
        ends = np.clip(np.asarray(offsets[:lim + 1], dtype=np.int64), 0, nk)
        for j in np.flatnonzero(ends[1:] > ends[:-1]):      # (an empty list gives +0: the zeros above)
            lo, hi = int(ends[j]), int(ends[j + 1])
            qs = [int(q) for q in slots[lo:hi]]
            if wrong == "descending":
                qs = qs[::-1]
            if wrong == "lose_entry" and len(qs) > 1:
                qs = qs[:-1]
            L = len(qs)
            q = np.asarray(qs, dtype=np.int64).reshape(L)
            ok = (q >= 0) & (q < nk)
            ok[ok] = row[q[ok]] == j
            qq = np.where(ok, q, 0)
            gq = gf[qq]
            has = ok & ((gq != 0) | (wrong == "no_zero_skip"))
            f = 2.0 * gq.astype(np.float64)                                       # exact
            e = x[qq // k, :3].astype(np.float64) - y[j, :3].astype(np.float64)[None, :]
            t64 = -f[:, None] * e
            if wrong == "sum_wide":
                tw = np.where(has[:, None], t64.astype(wide), wide(0))
                out[j, :3] = csum(tw, np.broadcast_to(has[:, None], (L, 3)), D).astype(T)
                continue
            terms, hh = t64.astype(T), np.broadcast_to(has[:, None], (L, 3))
            if wrong == "chunk_off_by_one":                 # a position without a term in front: every boundary moves by one
                terms, hh = np.concatenate([np.zeros((1, 3), dtype=T), terms]), np.concatenate([np.zeros((1, 3), dtype=bool), hh])
            out[j, :3] = csum(np.ascontiguousarray(terms), hh, D)
    return out


def knn_det_bound(g, idx, x, y, rows, dtype, D=DET_CHUNK):
    """-> (S (m, 3) long double, B (m, 3), deg (m,), By (m, 3) the atomic path's own bound, walk_layouts'): the exact gradient of y from the extended-precision terms (walk_layouts.knn_grad_terms)
    and the bound on knn_det_ref's distance from it, derived from the rule, with u the unit roundoff of T and A = sum |t| over a row's
    list of deg entries:
      a term is formed in double -- the difference and the product round, 2 * 2^-53 relative -- and rounded once to T: (1 + 2) u |t| at
      the most (float64: the rounding to T is exact, 2 u; float32: u (1 + 2^-28));
      a chunk holds min(deg, D) terms at the most and adds them from +0: min(deg, D) - 1 roundings that matter (0 + t is exact), each
      at most u times the running sum, itself at most A (1 + small);
      the ceil(deg / D) partials are added to a total from +0: ceil(deg / D) roundings at the most (none for a single chunk), each
      at most u A (1 + small).
    First order: (min(deg, D) - 1 + ceil(deg / D) + 3) u A; the one unit left over covers the second-order products -- about
    (D ceil(deg / D) + ceil(deg / D)^2 / 2) u^2 A, below u A while deg <= 2^18 (asserted) in float32 and float64.  Entries whose g is 0 have no
    term: queries all of whose cotangents are 0 may hold non-finite coordinates, which the exact evaluation replaces by 0."""
    u = wl.U[wl.np_dtype(dtype)]
    m = y.shape[0]
    lim = m if rows is None else min(max(int(rows), 0), m)
    live = ir.slot_rows(idx, m, rows)
    gz = np.where(live >= 0, g, 0)
    xs = np.where((gz != 0).any(1)[:, None], x[:, :3], 0)
    _, _, S, By, deg = wl.knn_grad_terms(xs, y[:, :3], live, gz, dtype)
    A = By / ((deg + 2) * u)[:, None]
    B = (np.minimum(deg, D) + -(-deg // D) + 3)[:, None] * u * A
    assert (deg[lim:] == 0).all() and deg.max(initial=0) <= 2 ** 18
    return S, B, deg, By


# ------------------------------------------------------------------ test inputs
def make_case(n, k, m, rows, degrees, dtype, seed, cx=3, cy=3):
    """One cloud's arguments with designed in-degrees (inverse_ref.make_degree_idx) -> a dict g (n, k), idx (n, k) int64, x (n, cx),
    y (m, cy), rows, offsets, slots.  Every fifth cotangent of a live slot is 0; one query with a live slot has all its cotangents 0
    and an inf coordinate (a["inf_query"]); the empty slots' cotangents are NaN and inf; the extra columns of x and y are NaN (never
    read)."""
    rng = np.random.default_rng(seed)
    idx = ir.make_degree_idx(n, k, m, degrees, seed)
    live = ir.slot_rows(idx, m, rows) >= 0
    g = ((rng.random((n, k)) + 0.5) * rng.choice([-1.0, 1.0], size=(n, k)) * 10.0 ** rng.integers(-2, 3, size=(n, k))).astype(dtype)
    g[rng.integers(0, 5, size=(n, k)) == 0] = 0
    x = np.full((n, cx), np.nan, dtype=dtype)
    y = np.full((m, cy), np.nan, dtype=dtype)
    x[:, :3] = (rng.random((n, 3)) * 2 - 1) * 10.0 ** rng.integers(-1, 2, size=(n, 1))
    y[:, :3] = (rng.random((m, 3)) * 2 - 1) * 10.0 ** rng.integers(-1, 2, size=(m, 1))
    iq = int(np.flatnonzero(live.any(1))[0]) if live.any() else -1
    if iq >= 0:
        g[iq], x[iq, 0] = 0, np.inf
    g = np.where(live, g, np.where(rng.integers(0, 2, size=(n, k)) == 0, np.nan, np.inf)).astype(dtype)
    off, slots = ir.invert_ref(idx, m, rows)
    return {"g": g, "idx": idx, "x": x, "y": y, "rows": rows, "offsets": off, "slots": slots, "inf_query": iq}


def ref_of(a, **kw):
    return knn_det_ref(a["g"], a["idx"], a["x"], a["y"], a["rows"], a["offsets"], a["slots"], **kw)
