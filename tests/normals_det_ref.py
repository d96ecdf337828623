"""The definition of the deterministic gradient of estimate_normals (deterministic=True) in numpy, for one cloud.

normals_det_ref restates dicp_amd/csrc/dicp_normals_det.h: per row j < rows the walk over the row's list in the inverted index of the
neighbour tensor (inverse_ref.invert_ref's, with the walk's clamps and its entry check), the term of each entry from the query's record
(G6[0:6], mu[6:9], p[9:12], f[12], all float64), and inverse_ref.chunked_sum's order of summation -- one numpy operation per rounding.  The
`wrong` keyword makes the deliberately wrong restatements that the tests show the comparison to refuse.  normals_det_bound gives the
exact sum of the terms in a wider type and what bounds the rule's distance from it.  A plain module (no fixtures): the tests put this
directory on sys.path and import it.
"""
import numpy as np

import inverse_ref as ir
from knn_det_ref import chunked_sum_fast
from dicp_amd.group import DET_CHUNK

REC = 13
WRONG = ("descending", "lose_entry", "term_for_f0", "no_mu", "chunk_off_by_one", "sum_wide")
SYM = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])          # G[a, c] = G6[SYM[a, c]]
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}


def terms64(R, y, no_mu=False):
    """R (L, 13) the entries' records, y (3,) float64 -> (L, 3) float64: the terms before their rounding to T, one numpy operation per
    rounding: d = (y - p) - mu, ((G_a0 d_0 + G_a1 d_1) + G_a2 d_2) f"""
    e = y[None, :] - R[:, 9:12]
    d = e if no_mu else e - R[:, 6:9]
    G = R[:, :6][:, SYM]                                    # (L, 3, 3)
    p0 = G[:, :, 0] * d[:, None, 0]
    p1 = G[:, :, 1] * d[:, None, 1]
    s1 = p0 + p1
    p2 = G[:, :, 2] * d[:, None, 2]
    s2 = s1 + p2
    return R[:, 12][:, None] * s2


def _lists(nbr, m, rows, offsets, slots):
    """the taken entries of every non-empty list: yields (j, q (L,) int64 with 0 where not taken, ok (L,) bool)"""
    k = nbr.shape[1]
    nk = m * k
    lim = m if rows is None else min(max(int(rows), 0), m)
    row = ir.slot_rows(nbr, m, rows).reshape(-1)
    ends = np.clip(np.asarray(offsets[:lim + 1], dtype=np.int64), 0, nk)
    for j in np.flatnonzero(ends[1:] > ends[:-1]):
        q = np.asarray(slots[int(ends[j]):int(ends[j + 1])], dtype=np.int64)
        ok = (q >= 0) & (q < nk)
        ok[ok] = row[q[ok]] == j
        yield int(j), np.where(ok, q, 0), ok


def normals_det_ref(rec, nbr, rows, offsets, slots, dtype, c=3, D=DET_CHUNK, wrong=None, fast=True):
    """rec (m, 13) float64, nbr (m, k) integer (original rows, anything else: empty), rows: the cloud's row count (None: m), offsets
    (m + 1,) and slots (m k,) the inverted index -> (m, c) in dtype.

    wrong: "descending" walks each list backwards; "lose_entry" drops the last entry of a list; "term_for_f0" gives an entry whose
    query has f = 0 its term (0 * inf = NaN behind an inf in G6); "no_mu" leaves mu out of d; "chunk_off_by_one" starts every chunk one
    position early; "sum_wide" sums the unrounded terms in a wider type (float64 for float32, long double for float64) and rounds at the
    end.  fast: knn_det_ref.chunked_sum_fast instead of inverse_ref.chunked_sum (the same bits, a chunk at a time)."""
    csum = chunked_sum_fast if fast else ir.chunked_sum
    T = np.dtype(dtype).type
    m, k = nbr.shape
    wide = np.float64 if T == np.float32 else np.longdouble
    out = np.zeros((m, c), dtype=T)
    with np.errstate(invalid="ignore", over="ignore"):
        for j, q, ok in _lists(nbr, m, rows, offsets, slots):
            if wrong == "descending":
                q, ok = q[::-1], ok[::-1]
            if wrong == "lose_entry" and q.size > 1:
                q, ok = q[:-1], ok[:-1]
            L = q.size
            R = rec[q // k]
            has = ok & ((R[:, 12] != 0) | (wrong == "term_for_f0"))
            t64 = terms64(R, rec[j, 9:12], no_mu=wrong == "no_mu")
            hh = np.broadcast_to(has[:, None], (L, 3))
            if wrong == "sum_wide":
                out[j, :3] = csum(np.where(hh, t64.astype(wide), wide(0)), hh, D).astype(T)
                continue
            terms = t64.astype(T)
            if wrong == "chunk_off_by_one":                 # a position without a term in front: every boundary moves by one
                terms, hh = np.concatenate([np.zeros((1, 3), dtype=T), terms]), np.concatenate([np.zeros((1, 3), dtype=bool), hh])
            out[j, :3] = csum(np.ascontiguousarray(terms), np.ascontiguousarray(hh), D)
    return out


def normals_det_bound(rec, nbr, rows, offsets, slots, dtype):
    """-> (S (m, 3) long double: the exact sum of the restatement's float64 terms, A (m, 3) long double: sum |term|, deg (m,): the list
    lengths, M (m, 3) long double: sum over the entries of f sum_c |G_ac| |d_c|, the scale of a term's own roundings).  The rule lies
    within (deg + 2) u_T A of S: a term is rounded once from double to T (u_T |t|; exact for float64); a list of deg entries in c chunks is
    added by deg - c additions that round inside the chunks and c - 1 between the partials (0 + t is exact), deg - 1 in all, each at
    most u_T times a running sum of at most A (1 + small): deg u_T A to first order with the term's rounding, and the two units left
    over cover the second-order products (about deg^2 u_T^2 A / 2) while deg u_T << 1."""
    m = nbr.shape[0]
    S, A, M, deg = np.zeros((m, 3), np.longdouble), np.zeros((m, 3), np.longdouble), np.zeros((m, 3), np.longdouble), np.zeros(m, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j, q, ok in _lists(nbr, m, rows, offsets, slots):
            R = rec[q // nbr.shape[1]]
            has = ok & (R[:, 12] != 0)
            t = terms64(R, rec[j, 9:12])[has].astype(np.longdouble)
            S[j], A[j], deg[j] = t.sum(0), np.abs(t).sum(0), q.size
            Ra = np.abs(R[has])
            Ra[:, 6:9] = 0                                  # |d| itself, from the rounded d: (y - p) - mu as the rule forms it
            e = rec[j, 9:12][None, :] - R[has][:, 9:12]
            Ra[:, 9:12] = -np.abs(e - R[has][:, 6:9])       # terms64 forms y - p: give it y = 0, p = -|d|
            M[j] = terms64(Ra, np.zeros(3)).astype(np.longdouble).sum(0)
    return S, A, deg, M


# ------------------------------------------------------------------ test inputs
def make_records(m, seed, zero_every=5, inf_query=None):
    """(m, 13) float64: G6, mu, p standard normal, f = 2 / k_eff for a k_eff in 3..32, f = 0 on every zero_every-th query (whose G6, mu
    stay random: a term formed for them would show); inf_query: an f = 0 query whose G6 holds an inf"""
    rng = np.random.default_rng(seed)
    rec = rng.standard_normal((m, REC))
    rec[:, 12] = 2.0 / rng.integers(3, 33, size=m)
    rec[rng.permutation(m)[:m // zero_every], 12] = 0.0
    if inf_query is not None:
        rec[inf_query, 12], rec[inf_query, 1] = 0.0, np.inf
    return rec


def make_case(m, k, rows, degrees, seed, idx_dtype=np.int64):
    """One cloud with designed in-degrees (inverse_ref.make_degree_idx) -> a dict rec (m, 13), nbr (m, k), rows, offsets, slots; the
    first query with a live slot has f = 0 and an inf in its G6 (a["inf_query"])"""
    nbr = ir.make_degree_idx(m, k, m, degrees, seed)
    live = ir.slot_rows(nbr, m, rows) >= 0
    iq = int(np.flatnonzero(live.any(1))[0]) if live.any() else None
    off, slots = ir.invert_ref(nbr, m, rows)
    return {"rec": make_records(m, seed + 1, inf_query=iq), "nbr": nbr.astype(idx_dtype), "rows": rows, "offsets": off, "slots": slots, "inf_query": iq}


def ref_of(a, dtype, **kw):
    return normals_det_ref(a["rec"], a["nbr"], a["rows"], a["offsets"], a["slots"], dtype, **kw)
