// The inverted index of a neighbour index tensor (dicp_amd/group.py: invert_neighbors) and the deterministic feature gradients that walk it
// (group_points / pool_neighbors / interpolate_features with deterministic=True): the per-element rules of csrc/inverse.hip.
//
// Plain inline C++ templated on the scalar T and the index type I, included by the HIP kernels and by a TEST-ONLY g++ build
// (tests/test_inverse_host.py) that runs the same lines in a serial loop and holds them to the numpy restatement tests/inverse_ref.py.
//
// Slot (i, s) of a cloud with n queries of k slots has the flat number q = i k + s; it is live when group_row(idx[q], rows) >= 0.  The
// index is two arrays per cloud: offsets (m + 1), offsets[j] = the live slots naming a row < j, and slots (n k), slots[offsets[j] :
// offsets[j + 1]] = the q of the live slots with idx = j in ASCENDING q, -1 past the live count.  The build sorts (key, q) stably by
// key = the row, or m for an empty slot, fed in ascending q.
//
// The gradient of destination element (j, c) is a sum over the list of row j in list order, in chunks of GROUP_DET_CHUNK list POSITIONS:
// each chunk is summed from +0 by plain additions, the chunks' partials p_0, p_1, ... are added in order to a total that starts at +0;
// a list of at most one chunk gives p_0 itself.  An entry without a term is skipped (its position still counts).  The walk never leaves
// its arrays whatever offsets / slots hold: both ends of a list are clamped to [0, n k], and an entry is taken only when its q is in
// range and idx[q] names row j.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dicp_group.h"

namespace dicp {

constexpr int GROUP_DET_CHUNK = 64;
static_assert(GROUP_DET_CHUNK >= 16 && GROUP_DET_CHUNK <= 256 && (GROUP_DET_CHUNK & (GROUP_DET_CHUNK - 1)) == 0, "a power of two in [16, 256]");

enum { DET_GROUP = 0, DET_POOL_SUM = 1, DET_POOL_MEAN = 2, DET_POOL_MAX = 3, DET_INTERP = 4 };

// ------------------------------------------------------------------ the build
// the sort key of a slot whose row is `row` (-1: empty): empty slots sort behind every row of the table
DICP_HD uint32_t inverse_key(int row, int m) { return row >= 0 ? (uint32_t)row : (uint32_t)m; }
// 8-bit digits that hold every key in [0, m], m >= 1
DICP_HD int inverse_passes(int m) {
    int bits = 0;
    for (uint32_t x = (uint32_t)m; x; x >>= 1) ++bits;
    return (bits + 7) / 8;
}
// sorted position p in [0, n k] of a cloud (position n k: past the end): the rows j whose offset is p are prev < j <= cur, prev the key
// before p (-1 at p = 0), cur the key at p (m past the end).  Every j in [0, m] belongs to exactly one p.
DICP_HD void inverse_offset_rows(const uint32_t* keys, int64_t p, int64_t nk, int m, int64_t& first, int64_t& last) {
    first = p > 0 ? (int64_t)keys[p - 1] + 1 : 0;
    last = p < nk ? (int64_t)keys[p] : (int64_t)m;
}

// ------------------------------------------------------------------ the walk
DICP_HD int det_clamp(int32_t x, int nk) { return x < 0 ? 0 : (x > nk ? nk : (int)x); }
// the list of row j of a cloud: positions [lo, hi) of its slots array, inside [0, n k] whatever the offsets hold (hi < lo: empty)
DICP_HD void det_list(const int32_t* offsets, int j, int nk, int& lo, int& hi) {
    lo = det_clamp(offsets[j], nk);
    hi = det_clamp(offsets[j + 1], nk);
    if (hi < lo) hi = lo;
}
// an entry is taken when its slot number is in range and the slot names row j (j < rows follows)
template <typename I>
DICP_HD bool det_entry(int32_t q, int nk, const I* idx, int rows, int j) { return (uint32_t)q < (uint32_t)nk && group_row(idx[q], rows) == j; }

DICP_HD bool det_chunk_start(int pos) { return pos > 0 && (pos & (GROUP_DET_CHUNK - 1)) == 0; }
template <typename T>
DICP_HD void det_flush(T& total, T& part) {
    total = total + part;
    part = T(0);
}
template <typename T>
DICP_HD T det_finish(T total, T part, int len) { return len <= GROUP_DET_CHUNK ? part : total + part; }

// slot s of query i of interpolate_features: false when the slot has no term (empty index or non-finite d2); otherwise w = r_s / R with
// r and R recomputed from the query's d2 row in slot order (an empty slot adds 0 to R: exact), as the forward does
template <typename T, typename I>
DICP_HD bool det_interp_weight(const I* idx, const T* d2, T eps, int i, int s, int k, int rows, T& w) {
    const size_t o = (size_t)i * k;
    T R = T(0), rs = T(0);
    bool on = false;
    for (int t = 0; t < k; ++t) {
        T r = T(0);
        if (group_row(idx[o + t], rows) >= 0) {
            const T d = d2[o + t];
            if (group_finite(d)) {
                r = interp_r<T>(d, eps);
                if (t == s) { rs = r; on = true; }
            }
        }
        R = R + r;
    }
    w = interp_w<T>(rs, R);
    return on;
}

// One cloud's arrays.  g: the cotangent, (n, k, C) for DET_GROUP and (n, C) otherwise; argmax (n, C): DET_POOL_MAX; counts (n): DET_POOL_MEAN;
// d2 (n, k), eps: DET_INTERP.
template <typename T, typename I>
struct DetCloud {
    const T* g;
    const I* idx;
    const int32_t* argmax;
    const int32_t* counts;
    const T* d2;
    T eps;
    int n, k, C, rows;
};

// out[0 .. V) = the gradient of elements (j, c .. c + V) of the feature table: V = 1, or a pack whose accesses are aligned to V elements
template <typename T, typename I, int V, int OP>
DICP_HD void det_row_sum(const DetCloud<T, I>& a, const int32_t* offsets, const int32_t* slots, int j, int c, T* out) {
    const int nk = a.n * a.k;
    int lo, hi;
    det_list(offsets, j, nk, lo, hi);
    T total[V], part[V];
#pragma unroll
    for (int v = 0; v < V; ++v) total[v] = part[v] = T(0);
    int last_i = -1;                                        // the query of the entry taken last: entries of one query are adjacent
    for (int e = lo; e < hi; ++e) {
        if (det_chunk_start(e - lo)) {
#pragma unroll
            for (int v = 0; v < V; ++v) det_flush<T>(total[v], part[v]);
        }
        const int32_t q = slots[e];
        if (!det_entry<I>(q, nk, a.idx, a.rows, j)) continue;
        const int i = q / a.k;
        const bool first = i != last_i;
        last_i = i;
        const T* gp = (const T*)__builtin_assume_aligned(a.g + (OP == DET_GROUP ? (size_t)q : (size_t)i) * a.C + c, sizeof(T) * V);
        if (OP == DET_GROUP || OP == DET_POOL_SUM) {
#pragma unroll
            for (int v = 0; v < V; ++v) part[v] = part[v] + gp[v];
        } else if (OP == DET_POOL_MEAN) {
            const int cnt = a.counts[i];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const T t = pool_mean_grad<T>(gp[v], cnt);
                part[v] = part[v] + t;
            }
        } else if (OP == DET_POOL_MAX) {
            if (!first) continue;                           // the atomic path adds once per (query, channel), however often the query names j
            const int32_t* am = a.argmax + (size_t)i * a.C + c;
#pragma unroll
            for (int v = 0; v < V; ++v)
                if (group_row(am[v], a.rows) == j) part[v] = part[v] + gp[v];
        } else {
            T w;
            if (!det_interp_weight<T, I>(a.idx, a.d2, a.eps, i, q - i * a.k, a.k, a.rows, w)) continue;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const T t = w * gp[v];
                part[v] = part[v] + t;
            }
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) out[v] = det_finish<T>(total[v], part[v], hi - lo);
}

}  // namespace dicp
