// The deterministic y-gradient of the neighbour searches (knn_points / ball_query / chamfer_distance with deterministic=True): the
// per-element rules of csrc/knn_det.hip, on the inverted index of the searches' public idx output (csrc/dicp_inverse.h).
//
// Plain inline C++ templated on the scalar T and the index type I, included by the HIP kernel and by a TEST-ONLY g++ build
// (tests/test_knn_det_host.py) that runs the same lines in a serial loop and holds them to the numpy restatement tests/knn_det_ref.py.
//
// Row l < rows of a cloud receives, per component a in 0..2, the sum over its list (the live slots q = i k + s with idx[q] = l, in
// ascending q) of the terms t_a = (T)(-(2.0 (double)g[q]) ((double)x[i, a] - (double)y[l, a])): the value the atomic kernels
// (knn_points_bwd_kernel, ball_bwd_kernel) add for that slot, rounded once to T.  An entry whose g is 0 has no term (the atomic kernels'
// own rule: it keeps 0 * inf out); its position still counts.  The order of summation is dicp_inverse.h's: chunks of GROUP_DET_CHUNK
// list positions, each summed from +0 by plain additions in T, the partials p_0, p_1, ... added in order to a total that starts at +0, a
// list of at most one chunk giving p_0 itself.  The term is formed in a statement of its own, so that -ffp-contract=on cannot fuse it
// into the sum.  The walk never leaves its arrays whatever offsets / slots hold: det_list's clamps and det_entry's check.
//
// Two forms of one rule.  knn_det_row_sum walks a list serially (a lane per row).  A list longer than KNN_DET_HUB chunks -- a hub: the
// one nearest target of thousands of Chamfer queries -- is summed by a whole wave instead: knn_det_chunk gives one chunk's partial from
// +0, and the partials are added in chunk order to a total that starts at +0 (knn_det_hub_sum is that fold in a serial loop).  For a
// list of more than one chunk the two are the same additions in the same order, so they give the same bits.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dicp_inverse.h"

namespace dicp {

// Lists of more than KNN_DET_HUB chunks are summed by their wave.  Origin of the value: see the note at the kernel (csrc/knn_det.hip).
#ifndef DICP_KNN_DET_HUB
#define DICP_KNN_DET_HUB 4
#endif
constexpr int KNN_DET_HUB = DICP_KNN_DET_HUB;
static_assert(KNN_DET_HUB >= 1, "a hub has more than one chunk: the fold of the partials is then det_finish's total + part");

// One cloud's arrays: g (n, k) the cotangent of d2, idx (n, k), x (n, cx) the queries; rows: the live rows of y
template <typename T, typename I>
struct KnnDetCloud {
    const T* g;
    const I* idx;
    const T* x;
    int cx, n, k, rows;
};

// the term of one component: 2 g exact in double, the difference and the product rounded in double, then once to T
template <typename T>
DICP_HD T knn_det_term(T g, T xa, T ya) {
    const double f = 2.0 * (double)g;
    const double e = (double)xa - (double)ya;
    const double t = -f * e;
    return (T)t;
}

// part[0..3) = part + the terms of list positions [e0, e1) of row j, in order; yr: the row's three coordinates.  KNN_DET_ILP entries
// at a time: their loads (the slot number, then idx and g, then the query row) do not depend on one another, so they are in flight
// together; an entry that is not taken reads slot 0 of the cloud instead (in range: n k >= 1) and its term is dropped.  The additions
// stay one per taken entry, in list order.
constexpr int KNN_DET_ILP = 8;
template <typename T, typename I>
DICP_HD void knn_det_entries(const KnnDetCloud<T, I>& a, const int32_t* slots, int j, const T* yr, int e0, int e1, T* part) {
    const int nk = a.n * a.k;
    for (int e = e0; e < e1; e += e1 - e > KNN_DET_ILP ? KNN_DET_ILP : e1 - e) {
        T t[KNN_DET_ILP][3];
        bool has[KNN_DET_ILP];
#pragma unroll
        for (int u = 0; u < KNN_DET_ILP; ++u) {
            const bool in_list = u < e1 - e;
            const int32_t q = slots[in_list ? e + u : e];
            const bool in_range = (uint32_t)q < (uint32_t)nk;
            const int32_t qq = in_range ? q : 0;
            const bool ok = in_list && in_range && det_entry<I>(qq, nk, a.idx, a.rows, j);
            const T g = a.g[qq];
            has[u] = ok && !(g == T(0));
            const T* xr = a.x + (size_t)(qq / a.k) * a.cx;
#pragma unroll
            for (int c = 0; c < 3; ++c) t[u][c] = knn_det_term<T>(g, xr[c], yr[c]);
        }
#pragma unroll
        for (int u = 0; u < KNN_DET_ILP; ++u) {
            if (!has[u]) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) part[c] = part[c] + t[u][c];
        }
    }
}

// chunk c of the list [lo, hi): its partial, summed from +0
template <typename T, typename I>
DICP_HD void knn_det_chunk(const KnnDetCloud<T, I>& a, const int32_t* slots, int j, const T* yr, int lo, int hi, int c, T* part) {
    part[0] = part[1] = part[2] = T(0);
    const int e0 = lo + c * GROUP_DET_CHUNK;                // (c < the list's chunks: e0 < hi <= n k < 2^31)
    const int e1 = hi - e0 > GROUP_DET_CHUNK ? e0 + GROUP_DET_CHUNK : hi;
    knn_det_entries<T, I>(a, slots, j, yr, e0, e1, part);
}

DICP_HD int knn_det_chunks(int lo, int hi) { return (hi - lo) / GROUP_DET_CHUNK + ((hi - lo) % GROUP_DET_CHUNK != 0); }
DICP_HD bool knn_det_is_hub(int lo, int hi) { return hi - lo > KNN_DET_HUB * GROUP_DET_CHUNK; }

// the serial form: out[0..3) = the gradient of row j's coordinates over the list [lo, hi) (det_list's)
template <typename T, typename I>
DICP_HD void knn_det_row_sum(const KnnDetCloud<T, I>& a, const int32_t* slots, int j, const T* yr, int lo, int hi, T* out) {
    T total[3] = {T(0), T(0), T(0)}, part[3] = {T(0), T(0), T(0)};
    const int chunks = knn_det_chunks(lo, hi);
    for (int ch = 0; ch < chunks; ++ch) {
        if (det_chunk_start(ch * GROUP_DET_CHUNK)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) det_flush<T>(total[c], part[c]);
        }
        const int e0 = lo + ch * GROUP_DET_CHUNK;           // (< hi <= n k < 2^31)
        knn_det_entries<T, I>(a, slots, j, yr, e0, hi - e0 > GROUP_DET_CHUNK ? e0 + GROUP_DET_CHUNK : hi, part);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = det_finish<T>(total[c], part[c], hi - lo);
}

// the hub form in a serial loop: the partials of the chunks added in chunk order to a total that starts at +0.  Equal to
// knn_det_row_sum for a list of more than one chunk (the kernel uses it only past KNN_DET_HUB chunks).
template <typename T, typename I>
DICP_HD void knn_det_hub_sum(const KnnDetCloud<T, I>& a, const int32_t* slots, int j, const T* yr, int lo, int hi, T* out) {
    T total[3] = {T(0), T(0), T(0)};
    const int chunks = knn_det_chunks(lo, hi);
    for (int c = 0; c < chunks; ++c) {
        T part[3];
        knn_det_chunk<T, I>(a, slots, j, yr, lo, hi, c, part);
#pragma unroll
        for (int v = 0; v < 3; ++v) total[v] = total[v] + part[v];
    }
    out[0] = total[0]; out[1] = total[1]; out[2] = total[2];
}

}  // namespace dicp
