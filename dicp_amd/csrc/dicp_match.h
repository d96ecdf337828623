// The exact k nearest rows in DESCRIPTOR space (dicp_amd/match.py: knn_features / match_features): the per-element rules of
// csrc/match.hip.
//
// Plain inline C++ templated on the scalar T, included by the HIP kernels and by a TEST-ONLY g++ build (tests/test_match_host.py) that
// runs the same lines in a serial loop and holds them bit for bit to the numpy restatement tests/match_ref.py.
//
// fma is the correctly rounded fused multiply-add of T (match_fma: v_fma_f32 / v_fma_f64 on the device, libm's on the host; the float32
// matrix-core form is held to the same chain by the GPU tests).  For rows x_i, y_j of D channels:
//   h_j        = T(0.5) q_j,  q = +0; for c = 0 .. D-1: q = fma(y_jc, y_jc, q)
//   score(i,j) : s = h_j;     for c = 0 .. D-1: s = fma(-x_ic, y_jc, s)              (= 0.5 (|x - y|^2 - |x|^2): the distance's order)
//   d2(i,j)    : r = +0;      for c = 0 .. D-1: t = x_ic - y_jc; r = fma(t, t, r)    (the winners only)
// The candidates of query i are the rows j < rows whose score is finite (a non-finite channel on either side leaves no finite score:
// such a row is nobody's neighbour and, as a query, gets none); the result is the first min(k, #candidates) of them in (score, index)
// order, and the slots keep that order.  d2 is recomputed from the differences: non-negative, exactly 0 for identical rows, free of the
// cancellation of |x|^2 + |y|^2 - 2 x.y; its order can differ from the score's at rounding level.
//
// The gradient of d2: the term of slot (i, s) naming row j is, per channel, t_c = (T)(2.0 (double)g_is ((double)x_ic - (double)y_jc)),
// rounded once; an entry with g == 0 or idx < 0 has no term.  gx[i, c] is the sum of the query's terms in slot order from +0; gy[j, c]
// the sum of -t_c (float atomics by default).  With deterministic=True gy[j, c] is summed over the row's list in the inverted index of
// idx in the order of csrc/dicp_inverse.h: chunks of GROUP_DET_CHUNK list positions, each from +0, the partials added in order to a total
// that starts at +0, a single chunk as it is (match_det_sum).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dicp_inverse.h"
#include "dicp_topk.h"

namespace dicp {

constexpr int MATCH_D_MAX = 256;
constexpr int MATCH_K_MAX = 32;
enum { MATCH_FORM_AUTO = 0, MATCH_FORM_VALU = 1, MATCH_FORM_MFMA = 2 };

DICP_HD float  match_fma(float a, float b, float c)    { return __builtin_fmaf(a, b, c); }
DICP_HD double match_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <typename T>
DICP_HD bool match_finite(T s) { return s - s == T(0); }                 // false for inf and NaN

template <typename T>
DICP_HD T match_half_norm(const T* y, int D) {
    T q = T(0);
    for (int c = 0; c < D; ++c) q = match_fma(y[c], y[c], q);
    return T(0.5) * q;
}

// one link of the score chain
template <typename T>
DICP_HD T match_score_step(T s, T x, T y) { return match_fma(-x, y, s); }

template <typename T>
DICP_HD T match_score(const T* x, const T* y, int D, T h) {
    T s = h;
    for (int c = 0; c < D; ++c) s = match_score_step<T>(s, x[c], y[c]);
    return s;
}

template <typename T>
DICP_HD T match_refine(const T* x, const T* y, int D) {
    T r = T(0);
    for (int c = 0; c < D; ++c) {
        const T t = x[c] - y[c];
        r = match_fma(t, t, r);
    }
    return r;
}

// the list of one query in a serial loop: sc / id (capacity K >= k, topk_init's layout: the list is entries K - k .. K - 1)
template <typename T, int K>
DICP_HD void match_query(const T* x, const T* y, const T* h, int rows, int D, int k, T (&sc)[K], int (&id)[K]) {
    int sl[K];
    topk_init<T, K>(sc, id, sl, k);
    const auto same = [](int j) { return j; };
    const auto ins = topk_inserter<T, K>(sc, id, sl, same);
    for (int j = 0; j < rows; ++j) {
        const T s = match_score<T>(x, y + (size_t)j * D, D, h[j]);
        if (match_finite<T>(s)) ins(s, j);
    }
}

// the outputs of list entry e: an empty entry (index -1) gives +inf / -1
template <typename T>
DICP_HD void match_output(const T* x, const T* y, int D, int j, T& d2, int64_t& idx) {
    if (j < 0) { d2 = static_cast<T>(__builtin_huge_val()); idx = -1; return; }
    d2 = match_refine<T>(x, y + (size_t)j * D, D);
    idx = j;
}

// ------------------------------------------------------------------ the gradient
template <typename T>
DICP_HD T match_term(T g, T x, T y) {
    const double f = 2.0 * (double)g;
    const double e = (double)x - (double)y;
    const double t = f * e;
    return (T)t;
}

// gx[i, c]: the query's terms in slot order from +0; g / idx: the k slots of the query; y: the cloud's table (m, D)
template <typename T>
DICP_HD T match_grad_x(const T* g, const int64_t* idx, int k, T xc, const T* y, int D, int m, int c) {
    T sum = T(0);
    for (int s = 0; s < k; ++s) {
        const int j = group_row(idx[s], m);
        if (j < 0 || g[s] == T(0)) continue;
        const T t = match_term<T>(g[s], xc, y[(size_t)j * D + c]);
        sum = sum + t;
    }
    return sum;
}

// gy[j, c] with deterministic=True: the list [lo, hi) of row j (det_list's) of slots, one cloud's g (n k), idx (n k), x (n, D)
template <typename T>
DICP_HD T match_det_sum(const T* g, const int64_t* idx, const T* x, int n, int k, int D, int rows, const int32_t* slots, int j, T yc, int c,
                        int lo, int hi) {
    const int nk = n * k;
    T total = T(0), part = T(0);
    for (int e = lo; e < hi; ++e) {
        if (det_chunk_start(e - lo)) det_flush<T>(total, part);
        const int32_t q = slots[e];
        if (!det_entry<int64_t>(q, nk, idx, rows, j)) continue;
        const T gq = g[q];
        if (gq == T(0)) continue;
        const T t = -match_term<T>(gq, x[(size_t)(q / k) * D + c], yc);
        part = part + t;
    }
    return det_finish<T>(total, part, hi - lo);
}

}  // namespace dicp
