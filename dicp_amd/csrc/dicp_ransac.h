// RANSAC over explicit correspondences (dicp_amd/match.py: ransac_correspondences / correspondence_residuals): the per-element rules of
// csrc/ransac.hip.
//
// Plain inline C++ templated on the scalar T, included by the HIP kernels and by a TEST-ONLY g++ build (tests/test_ransac_host.py) that
// runs the same lines in a serial loop and holds them to the numpy restatement tests/ransac_ref.py.
//
// A cloud's live pairs are packed (x_i[0:3], y_j[0:3]) rows of 6 values of T, P of them, in ascending i.
//   sample of hypothesis h (integers only, 32-bit wrap-around; mix32 is the hash of kernels_soft_svd.h):
//       kc = mix32(seed ^ cloud 0x9E3779B9), kh = mix32(kc ^ h 0x85EBCA6B), u_t = mix32(kh ^ (t 0xC2B2AE35 + 0x27D4EB2F)), t = 0, 1, 2
//       mulhi(u, q) = (u q) >> 32 on the 64-bit product
//       a = mulhi(u0, P); b = mulhi(u1, P - 1), b += (b >= a); c = mulhi(u2, P - 2), c += (c >= min(a, b)), c += (c >= max(a, b))
//     three distinct positions below P (P >= 3).
//   minimal fit, in double: the 18 Kabsch sums of dicp_math.h start at 0, the pairs a, b, c are added in that order at weight 1, then
//     kabsch_forward (proper rotation, rank-deficient completion); C (9, row-major) and r (3) are rounded once to T: the pose (12).
//   residual of a pair under a pose in T, fma = match_fma:
//       q_a = fma(C_a2, x_2, fma(C_a1, x_1, fma(C_a0, x_0, r_a))), e_a = q_a - y_a;  d = +0, d = fma(e_a, e_a, d) for a = 0, 1, 2
//     the pair is an inlier iff d <= thr2, thr2 = T((double)threshold (double)threshold); a NaN d never is.
//   choice: the hypothesis with the largest count, ties to the lowest h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dicp_match.h"

namespace dicp {

constexpr int RANSAC_H_MAX = 65536;
constexpr int RANSAC_ROW = 6;           // values of a packed pair: x[0:3], y[0:3]

DICP_HD uint32_t ransac_mix32(uint32_t v) {
    v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;
    return v;
}

DICP_HD uint32_t ransac_mulhi(uint32_t u, uint32_t q) { return (uint32_t)(((uint64_t)u * (uint64_t)q) >> 32); }

// three distinct positions below P from three 32-bit draws; P >= 3
DICP_HD void ransac_positions(uint32_t u0, uint32_t u1, uint32_t u2, uint32_t P, int32_t& a, int32_t& b, int32_t& c) {
    const uint32_t pa = ransac_mulhi(u0, P);
    uint32_t pb = ransac_mulhi(u1, P - 1u);
    pb += pb >= pa ? 1u : 0u;
    const uint32_t lo = pa < pb ? pa : pb, hi = pa < pb ? pb : pa;
    uint32_t pc = ransac_mulhi(u2, P - 2u);
    pc += pc >= lo ? 1u : 0u;
    pc += pc >= hi ? 1u : 0u;
    a = (int32_t)pa; b = (int32_t)pb; c = (int32_t)pc;
}

DICP_HD void ransac_draws(uint32_t seed, uint32_t cloud, uint32_t h, uint32_t& u0, uint32_t& u1, uint32_t& u2) {
    const uint32_t kc = ransac_mix32(seed ^ (cloud * 0x9E3779B9u));
    const uint32_t kh = ransac_mix32(kc ^ (h * 0x85EBCA6Bu));
    u0 = ransac_mix32(kh ^ (0u * 0xC2B2AE35u + 0x27D4EB2Fu));
    u1 = ransac_mix32(kh ^ (1u * 0xC2B2AE35u + 0x27D4EB2Fu));
    u2 = ransac_mix32(kh ^ (2u * 0xC2B2AE35u + 0x27D4EB2Fu));
}

DICP_HD void ransac_sample(uint32_t seed, uint32_t cloud, uint32_t h, uint32_t P, int32_t& a, int32_t& b, int32_t& c) {
    uint32_t u0, u1, u2;
    ransac_draws(seed, cloud, h, u0, u1, u2);
    ransac_positions(u0, u1, u2, P, a, b, c);
}

// one packed pair into the 18 sums at weight 1
template <typename T>
DICP_HD void ransac_add_pair(double (&acc)[NKAB], const T* row) {
    const double p[3] = {(double)row[0], (double)row[1], (double)row[2]};
    const double y[3] = {(double)row[3], (double)row[4], (double)row[5]};
    acc[KAB_S0] += 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        acc[KAB_SP + a] += p[a];
        acc[KAB_SY + a] += y[a];
#pragma unroll
        for (int b = 0; b < 3; ++b) acc[KAB_M + a * 3 + b] += y[a] * p[b];
    }
    acc[KAB_PP] += dot3(p, p);
    acc[KAB_YY] += dot3(y, y);
}

// the sums of a sample: from 0, the rows in the order given
template <typename T>
DICP_HD void ransac_sums(const T* ra, const T* rb, const T* rc, double (&acc)[NKAB]) {
#pragma unroll
    for (int i = 0; i < NKAB; ++i) acc[i] = 0.0;
    ransac_add_pair<T>(acc, ra);
    ransac_add_pair<T>(acc, rb);
    ransac_add_pair<T>(acc, rc);
}

// the pose (C row-major, then r) of a sample, rounded once to T
template <typename T>
DICP_HD void ransac_fit(const T* ra, const T* rb, const T* rc, T (&pose)[12]) {
    double acc[NKAB], C[9], r[3], save[KAB_SAVE];
    ransac_sums<T>(ra, rb, rc, acc);
    kabsch_forward(acc, C, r, save);
#pragma unroll
    for (int i = 0; i < 9; ++i) pose[i] = (T)C[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) pose[9 + i] = (T)r[i];
}

// d of the pair (x, y) under the pose
template <typename T>
DICP_HD T ransac_residual(const T (&pose)[12], T x0, T x1, T x2, T y0, T y1, T y2) {
    const T q0 = match_fma(pose[2], x2, match_fma(pose[1], x1, match_fma(pose[0], x0, pose[9])));
    const T q1 = match_fma(pose[5], x2, match_fma(pose[4], x1, match_fma(pose[3], x0, pose[10])));
    const T q2 = match_fma(pose[8], x2, match_fma(pose[7], x1, match_fma(pose[6], x0, pose[11])));
    const T e0 = q0 - y0, e1 = q1 - y1, e2 = q2 - y2;
    T d = T(0);
    d = match_fma(e0, e0, d);
    d = match_fma(e1, e1, d);
    d = match_fma(e2, e2, d);
    return d;
}

template <typename T>
DICP_HD bool ransac_inlier(T d, T thr2) { return d <= thr2; }            // false for NaN

template <typename T>
DICP_HD T ransac_thr2(double threshold) { return (T)(threshold * threshold); }

// (count, h) order: does (ca, ha) come before (cb, hb)?  The larger count, then the lower h
DICP_HD bool ransac_better(int32_t ca, int32_t ha, int32_t cb, int32_t hb) { return ca > cb || (ca == cb && ha < hb); }

// is a pair live?  i < rows, idx >= 0, all six values finite (the caller clamps idx into [0, m - 1] before it reads y)
template <typename T>
DICP_HD bool ransac_live(bool in_rows, int64_t idx, const T* x, const T* y) {
    return in_rows && idx >= 0 && match_finite<T>(x[0]) && match_finite<T>(x[1]) && match_finite<T>(x[2]) && match_finite<T>(y[0]) &&
           match_finite<T>(y[1]) && match_finite<T>(y[2]);
}

}  // namespace dicp
