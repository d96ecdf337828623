"""The definition of dicp_amd.group.invert_neighbors and of the deterministic feature gradients in numpy, for one cloud.

invert_ref restates invert_neighbors' docstring: a stable sort of the live slots by the row they name.  chunked_sum restates the order of
summation of a list (chunks of D list positions, each from +0, the partials added in order to a total that starts at +0), and det_grad_ref
each operator's deterministic gradient into the feature table: the walk over a row's list with its clamps and its entry check, the term of
each entry, one numpy operation per rounding in the table's dtype T.  D is read from the package (dicp_amd.group.DET_CHUNK).  The `wrong`
keyword makes the deliberately wrong restatements that the tests show the comparison to refuse.  Built on group_ref.  A plain module (no
fixtures): the tests put this directory on sys.path and import it.
"""
import numpy as np

import group_ref as gr
from dicp_amd.group import DET_CHUNK

OPS = ("group", "sum", "mean", "max", "interp")
WRONG = ("descending", "lose_entry", "max_counts_duplicates", "truncate_index")


def slot_rows(idx, m, rows=None, truncate=False):
    """(n, k) int64: the row every slot names, -1 for an empty slot: 0 <= idx < rows on the index's full width.  truncate: the wrong
    rule that looks at the low 32 bits only"""
    lim = m if rows is None else min(max(int(rows), 0), m)
    v = idx.astype(np.int64)
    if truncate:
        v = v & 0xFFFFFFFF
        v = np.where(v >= 2 ** 31, v - 2 ** 32, v)
    return np.where((v >= 0) & (v < lim), v, -1)


def invert_ref(idx, m, rows=None, truncate=False):
    """-> offsets (m + 1,) int32, slots (n k,) int32.  truncate: slot_rows' wrong rule"""
    row = slot_rows(idx, m, rows, truncate).reshape(-1)
    q = np.flatnonzero(row >= 0)
    order = q[np.argsort(row[q], kind="stable")]            # ascending row, ascending q within a row
    slots = np.full(row.size, -1, dtype=np.int32)
    slots[:order.size] = order
    offsets = np.zeros(m + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(np.bincount(row[q], minlength=m)[:m])
    return offsets, slots


def chunked_sum(terms, has, D=DET_CHUNK):
    """terms (L, C) in dtype T, has (L, C) bool (an entry without a term is skipped; its position counts) -> (C,) in T"""
    T = terms.dtype.type
    L, C = terms.shape
    total, part = np.zeros(C, dtype=T), np.zeros(C, dtype=T)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(L):
            if e > 0 and e % D == 0:
                total = (total + part).astype(T)
                part = np.zeros(C, dtype=T)
            part = np.where(has[e], (part + terms[e]).astype(T), part)
        return part if L <= D else (total + part).astype(T)


def det_grad_ref(op, g, idx, m, rows, offsets, slots, argmax=None, counts=None, d2=None, eps=None, D=DET_CHUNK, wrong=None):
    """-> (m, C) in g's dtype: the gradient of the feature table of one cloud.

    g: (n, k, C) for "group", (n, C) otherwise.  argmax (n, C): "max"; counts (n,): "mean"; d2 (n, k), eps: "interp"."""
    T = g.dtype.type
    n, k = idx.shape
    nk, C = n * k, g.shape[-1]
    lim = m if rows is None else min(max(int(rows), 0), m)
    row = slot_rows(idx, m, rows, truncate=wrong == "truncate_index").reshape(-1)
    if op == "interp":
        live, r, R, w = gr._interp_weights(idx, d2, T(eps), m, rows, T)
    out = np.zeros((m, C), dtype=T)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(m):
            lo, hi = (min(max(int(offsets[j + t]), 0), nk) for t in (0, 1))
            hi = max(hi, lo)
            qs = [int(x) for x in slots[lo:hi]]
            if wrong == "descending":
                qs = qs[::-1]
            if wrong == "lose_entry" and len(qs) > 1:
                qs = qs[:-1]
            terms, has = np.zeros((len(qs), C), dtype=T), np.zeros((len(qs), C), dtype=bool)
            last_i = -1
            for e, q in enumerate(qs):
                if not (0 <= q < nk and row[q] == j):
                    continue
                i, s = divmod(q, k)
                first, last_i = i != last_i, i
                if op == "group":
                    terms[e], has[e] = g[i, s], True
                elif op == "sum":
                    terms[e], has[e] = g[i], True
                elif op == "mean":
                    terms[e], has[e] = (g[i] / T(counts[i])).astype(T), True
                elif op == "max":
                    if first or wrong == "max_counts_duplicates":
                        a = argmax[i].astype(np.int64)
                        terms[e], has[e] = g[i], (a == j) & (a >= 0) & (a < lim)
                else:
                    if live[i, s]:
                        terms[e], has[e] = (w[i, s] * g[i]).astype(T), True
            out[j] = chunked_sum(terms, has, D)
    return out


# ------------------------------------------------------------------ test inputs
def make_idx(n, k, m, rows, seed, dtype=np.int64):
    """group_ref.make_idx (every kind of slot) with, in addition: queries that name one row in several slots, and -- int64 only -- values
    whose low 32 bits are a live row but which are not one"""
    rng = np.random.default_rng(seed + 1000)
    idx = gr.make_idx(n, k, m, rows, seed, np.int64)
    if k >= 2 and rows >= 1:
        dup = np.arange(n) % 4 == 2
        idx[dup, 1] = idx[dup, 0]
        if k >= 3:
            idx[dup, k - 1] = idx[dup, 0]                   # not adjacent in the query either
    if dtype == np.int64 and rows >= 1:
        far = rng.integers(0, 7, size=(n, k)) == 0
        idx = np.where(far, (rng.integers(1, 2 ** 20, size=(n, k)) << 32) + rng.integers(0, max(rows, 1), size=(n, k)), idx)
    return idx.astype(dtype)


def idx_kinds(idx, m, rows):
    """what make_idx promises beyond group_ref.idx_kinds"""
    row = slot_rows(idx, m, rows)
    srt = np.sort(row, axis=1)
    return {"duplicate_in_query": bool(((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any()) if idx.shape[1] > 1 else True,
            "low_bits_live": bool((slot_rows(idx, m, rows, truncate=True) != row).any()) if idx.dtype == np.int64 else True}


def make_degree_idx(n, k, m, degrees, seed):
    """(n, k) int64 in which row j is named by exactly degrees[j] slots for the rows of the dict `degrees`, the slots spread over the
    queries in a random order; every other slot is -1"""
    rng = np.random.default_rng(seed)
    assert sum(degrees.values()) <= n * k
    flat = np.full(n * k, -1, dtype=np.int64)
    pos = rng.permutation(n * k)
    at = 0
    for j, d in degrees.items():
        flat[pos[at:at + d]] = j
        at += d
    return flat.reshape(n, k)
