// Spatial compatibility of correspondences (dicp_amd/match.py: correspondence_compatibility / prune_correspondences): the per-element
// rules of csrc/compat.hip.
//
// Plain inline C++ templated on the scalar T, included by the HIP kernels and by a TEST-ONLY g++ build (tests/test_compat_host.py) that
// runs the same lines in a serial loop and holds them bit for bit to the numpy restatement tests/compat_ref.py.
//
// A cloud's live pairs are ransac_correspondences' (dicp_ransac.h: ransac_live, the clamp of idx, packed in ascending row order): P rows
// (x[0:3], y[0:3]) of 6 values of T.  fma = match_fma; sqrt and / are the correctly rounded ones of T.
//   compatibility of packed positions p != q:
//       t_a = x_pa - x_qa,  A = +0, A = fma(t_a, t_a, A) for a = 0, 1, 2;  B likewise from y;  a = sqrt(A), b = sqrt(B), e = a - b;
//       compatible iff e <= thr and e >= -thr and a >= L and b >= L, thr = T(threshold), L = T(min_length): false whenever a NaN is
//       compared.  t only changes sign when p and q swap, so the relation is symmetric bit for bit.
//   degree_p = the number of q != p below P compatible with p.
//   score: v^0 = 1; for t = 1 .. iterations: w_p = +0, then for q = 0 .. P - 1 in ascending order w_p = w_p + v_q where q is compatible
//       with p or q == p (one rounding per addition; the terms are >= +0, so adding +0 for the others leaves the same bits);
//       wmax = max_p w_p (>= 1 for P >= 1);  v_p = w_p / wmax.  score = v^iterations.
//   rank_p = the number of q below P with score_q > score_p, or score_q == score_p and q < p.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dicp_match.h"

namespace dicp {

constexpr int COMPAT_ITER_MAX = 64;
constexpr int COMPAT_ROW = 6;           // values of a packed pair: x[0:3], y[0:3] (RANSAC_ROW)

DICP_HD float  compat_sqrt(float a)  { return __builtin_sqrtf(a); }
DICP_HD double compat_sqrt(double a) { return __builtin_sqrt(a); }

template <typename T>
DICP_HD T compat_thr(double threshold) { return (T)threshold; }

// A (or B): the squared length of the difference of two points, one fma chain from +0
template <typename T>
DICP_HD T compat_len2(T p0, T p1, T p2, T q0, T q1, T q2) {
    const T t0 = p0 - q0, t1 = p1 - q1, t2 = p2 - q2;
    T s = T(0);
    s = match_fma(t0, t0, s);
    s = match_fma(t1, t1, s);
    s = match_fma(t2, t2, s);
    return s;
}

// e = a - b with a = sqrt(A), b = sqrt(B)
template <typename T>
DICP_HD T compat_error(T A, T B, T& a, T& b) {
    a = compat_sqrt(A);
    b = compat_sqrt(B);
    return a - b;
}

// |e| <= thr and a >= L and b >= L; every comparison with a NaN is false
template <typename T>
DICP_HD bool compat_holds(T e, T a, T b, T thr, T L) { return e <= thr && e >= -thr && a >= L && b >= L; }

// are the packed rows rp and rq (6 values each) compatible?
template <typename T>
DICP_HD bool compat_pair(T px0, T px1, T px2, T py0, T py1, T py2, T qx0, T qx1, T qx2, T qy0, T qy1, T qy2, T thr, T L) {
    const T A = compat_len2<T>(px0, px1, px2, qx0, qx1, qx2);
    const T B = compat_len2<T>(py0, py1, py2, qy0, qy1, qy2);
    T a, b;
    const T e = compat_error<T>(A, B, a, b);
    return compat_holds<T>(e, a, b, thr, L);
}

// what position q adds to w_p: v_q for a compatible q and for q == p (the self term), +0 otherwise
template <typename T>
DICP_HD T compat_term(bool same, bool compatible, T v) { return (same || compatible) ? v : T(0); }

// v = w / wmax
template <typename T>
DICP_HD T compat_div(T w, T wmax) { return w / wmax; }

// (score, position) order: does (sq, q) come before (sp, p)?  The larger score, then the lower position
template <typename T>
DICP_HD bool compat_before(T sq, int q, T sp, int p) { return sq > sp || (sq == sp && q < p); }

}  // namespace dicp
