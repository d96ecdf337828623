// Soft descriptor matches (dicp_amd/match.py: soft_match_features): the per-element rules of csrc/softmatch.hip.
//
// Plain inline C++ templated on the scalar T, included by the HIP kernels and by a TEST-ONLY g++ build (tests/test_softmatch_host.py) that
// runs the same lines in a serial loop and holds them to the float64 reference tests/softmatch_ref.py within its error model.
//
// The score s_ij and its candidates are csrc/dicp_match.h's, bit for bit.  With c = (T)(-2.0 / tau), rounded once on the host:
//   l_ij = c s_ij (one rounding),  p_ij = exp(l_ij - lse_i) over the candidates,  out_i = sum_j p_ij values_j,
//   idx_i = the first candidate in (score, index) order,  prob_i = p_{i, idx_i}.
// s_ij = 0.5 (|x - y|^2 - |x|^2), so p is softmax_j(-|x_i - y_j|^2 / tau): the per-query constant cancels.
//
// The forward is an ONLINE softmax in blocks of up to SOFT_ROWS rows: the block's largest logit raises the running maximum M once
// (soft_raise: S and the C sums are multiplied by exp(M - M'), skipped when the maximum stays: the factor would be exactly 1), then every
// candidate of the block adds e = exp(l - M) to S and e values_jk to the sums by fma (soft_add).  A row that is no candidate is skipped by a
// predicate, never by its value: a pad row's values are not read into any sum.  Two states of one query (the matrix-core form keeps the
// two halves of every tile on two lanes) are joined by soft_merge; soft_finish divides, and writes lse = M + log S.  A query without a
// candidate gets a zero row, idx -1, prob 0 and lse = +inf, the mark by which the backward passes skip it whatever its cotangent holds.
//
// float32 on the device uses the one-instruction forms (__expf, __logf, v_rcp_f32: csrc/dicp_math.h); float64 and the host build the
// library's.
//
// The backward recomputes s by the same chain and p = exp(c s - lse) (soft_prob).  With g the cotangent of out, delta_i = g_i . out_i and
// a_ij = p_ij (g_i . values_j - delta_i):
//   gfx_ic     = (-c) sum_j a_ij y_jc                               (one pass owns the queries)
//   gfy_jc     = c (y_jc sum_i a_ij - sum_i a_ij x_ic)              (one pass owns the rows of fy)
//   gvalues_jk = sum_i p_ij g_ik
// every sum sequential from +0 by fma -- in ascending index on the vector unit, in the tiles' register order in the matrix-core backward
// (csrc/softmatch.hip) --; every element stored once.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "dicp_match.h"

namespace dicp {

constexpr int SOFT_C_MAX = 8;
constexpr int SOFT_ROWS = 16;           // rows per block of the online softmax

#if defined(__HIP_DEVICE_COMPILE__)
DICP_HD float  soft_exp(float v)  { return __expf(v); }
DICP_HD float  soft_log(float v)  { return __logf(v); }
DICP_HD float  soft_rcp(float v)  { return __builtin_amdgcn_rcpf(v); }
#else
DICP_HD float  soft_exp(float v)  { return expf(v); }
DICP_HD float  soft_log(float v)  { return logf(v); }
DICP_HD float  soft_rcp(float v)  { return 1.0f / v; }
#endif
DICP_HD double soft_exp(double v) { return exp(v); }
DICP_HD double soft_log(double v) { return log(v); }
DICP_HD double soft_rcp(double v) { return 1.0 / v; }

template <typename T> DICP_HD T soft_inf() { return static_cast<T>(__builtin_huge_val()); }
template <typename T> DICP_HD T soft_scale(double tau) { return (T)(-2.0 / tau); }
template <typename T> DICP_HD T soft_logit(T c, T s) { return c * s; }

// the online state of one query (or of one of its two lanes): CC >= C sums, the columns past C stay +0
template <typename T, int CC>
struct SoftState {
    T M, S, a[CC];
    T bs;               // the smallest score so far and its row
    int bj;
};

template <typename T, int CC>
DICP_HD void soft_init(SoftState<T, CC>& q) {
    q.M = -soft_inf<T>();
    q.S = T(0);
#pragma unroll
    for (int k = 0; k < CC; ++k) q.a[k] = T(0);
    q.bs = soft_inf<T>();
    q.bj = -1;
}

// a block whose largest candidate logit is Mb (-inf: the block has none) begins
template <typename T, int CC>
DICP_HD void soft_raise(SoftState<T, CC>& q, T Mb) {
    if (!(Mb > q.M)) return;
    const T sc = soft_exp(q.M - Mb);            // M = -inf the first time: exp(-inf) = 0 on sums that are 0
    q.S = q.S * sc;
#pragma unroll
    for (int k = 0; k < CC; ++k) q.a[k] = q.a[k] * sc;
    q.M = Mb;
}

// candidate row j with score s, logit l <= q.M and values v[0 .. CC)
template <typename T, int CC>
DICP_HD void soft_add(SoftState<T, CC>& q, T s, T l, int j, const T* v) {
    const T e = soft_exp(l - q.M);
    q.S = q.S + e;
#pragma unroll
    for (int k = 0; k < CC; ++k) q.a[k] = match_fma(e, v[k], q.a[k]);
    if (s < q.bs || (s == q.bs && j < q.bj)) { q.bs = s; q.bj = j; }
}

// q takes the rows of o
template <typename T, int CC>
DICP_HD void soft_merge(SoftState<T, CC>& q, const SoftState<T, CC>& o) {
    if (o.bj < 0) return;
    soft_raise<T, CC>(q, o.M);
    const T f = soft_exp(o.M - q.M);
    q.S = match_fma(o.S, f, q.S);
#pragma unroll
    for (int k = 0; k < CC; ++k) q.a[k] = match_fma(o.a[k], f, q.a[k]);
    if (o.bs < q.bs || (o.bs == q.bs && o.bj < q.bj)) { q.bs = o.bs; q.bj = o.bj; }
}

template <typename T, int CC>
DICP_HD void soft_finish(const SoftState<T, CC>& q, T c, T* out, T& lse, int64_t& idx, T& prob) {
    if (q.bj < 0) {
#pragma unroll
        for (int k = 0; k < CC; ++k) out[k] = T(0);
        lse = soft_inf<T>();
        idx = -1;
        prob = T(0);
        return;
    }
    const T inv = soft_rcp(q.S);
#pragma unroll
    for (int k = 0; k < CC; ++k) out[k] = q.a[k] * inv;
    lse = q.M + soft_log(q.S);
    idx = q.bj;
    prob = soft_exp(soft_logit<T>(c, q.bs) - lse);
}

// ------------------------------------------------------------------ the gradient
template <typename T> DICP_HD bool soft_live(T lse) { return lse < soft_inf<T>(); }        // false for the mark of a query without candidates
template <typename T> DICP_HD T soft_prob(T c, T s, T lse) { return soft_exp(soft_logit<T>(c, s) - lse); }

template <typename T, int CC>
DICP_HD T soft_dot(const T* g, const T* v) {
    T d = T(0);
#pragma unroll
    for (int k = 0; k < CC; ++k) d = match_fma(g[k], v[k], d);
    return d;
}

template <typename T> DICP_HD T soft_a(T p, T gv, T delta) { return p * (gv - delta); }
template <typename T> DICP_HD T soft_grad_x(T c, T G) { return (-c) * G; }
template <typename T> DICP_HD T soft_grad_y(T c, T y, T sa, T A) { return c * match_fma(y, sa, -A); }

// ------------------------------------------------------------------ serial restatements (the host check; the vector kernels walk the same order)
// the forward of one query: rows of fy in blocks of SOFT_ROWS
template <typename T, int CC>
DICP_HD void soft_query(const T* x, const T* y, const T* h, const T* values, int rows, int D, int C, T c, T* out, T& lse, int64_t& idx, T& prob) {
    SoftState<T, CC> q;
    soft_init<T, CC>(q);
    for (int base = 0; base < rows; base += SOFT_ROWS) {
        const int nr = rows - base < SOFT_ROWS ? rows - base : SOFT_ROWS;
        T s[SOFT_ROWS], l[SOFT_ROWS], Mb = -soft_inf<T>();
        for (int r = 0; r < nr; ++r) {
            s[r] = match_score<T>(x, y + (size_t)(base + r) * D, D, h[base + r]);
            l[r] = soft_logit<T>(c, s[r]);
            if (match_finite<T>(s[r]) && l[r] > Mb) Mb = l[r];
        }
        soft_raise<T, CC>(q, Mb);
        for (int r = 0; r < nr; ++r) {
            if (!match_finite<T>(s[r])) continue;
            T v[CC];
            for (int k = 0; k < CC; ++k) v[k] = k < C ? values[(size_t)(base + r) * C + k] : T(0);
            soft_add<T, CC>(q, s[r], l[r], base + r, v);
        }
    }
    T o[CC];
    soft_finish<T, CC>(q, c, o, lse, idx, prob);
    for (int k = 0; k < C; ++k) out[k] = o[k];
}

}  // namespace dicp
