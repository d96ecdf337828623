// What the translation units of the surface normals share (csrc/normals.hip, csrc/normals_det.hip): the layouts of the forward workspaces,
// the two layouts of a cloud's sorted rows (the x-sorted walk, the cell grid), the per-point eigen-system and the argument checks.
// Internal linkage, like dicp_common.h: each .hip file gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_normals.h"
#include "kernels_grid_plan.h"

namespace {

constexpr int NRM_KMAX = 32;
template <typename T> struct NrmTau;
template <> struct NrmTau<float>  { static constexpr double v = 1e-6; };
template <> struct NrmTau<double> { static constexpr double v = 1e-12; };

// The forward workspace, in this order (each part 256-byte aligned); the backward reads tperm / tgs4 / nbr_s of it
struct NrmLayout {
    size_t xyz, keys, tperm, tgs4, nbr_s, scratch, scratch_bytes, total;
};
inline NrmLayout nrm_layout(int dtype, int N, int m, int k) {
    NrmLayout L;
    const size_t ts = elem_size(dtype), m_pad = (size_t)dicp_padded_targets(m);
    size_t off = 0;
    L.xyz = off;     off = up256(off + (size_t)N * m * 3 * ts);
    L.keys = off;    off = up256(off + (size_t)N * m_pad * ts);
    L.tperm = off;   off = up256(off + (size_t)N * m_pad * 4);
    L.tgs4 = off;    off = up256(off + (size_t)N * m_pad * 4 * ts);
    L.nbr_s = off;   off = up256(off + (size_t)N * m_pad * k * 4);
    L.scratch_bytes = dicp_sweep_sort_scratch_bytes(dtype, N, (int)m_pad);
    L.scratch = off; off = up256(off + L.scratch_bytes);
    L.total = off;
    return L;
}

// The forward workspace of method="grid" (each part 256-byte aligned); the backward reads plans / perm / rows4 / nbr_s of it
struct NrmGridLayout {
    size_t plans, keys, perm, rows4, nbr_s, total;
};
inline NrmGridLayout nrm_grid_layout(int dtype, int N, int m, int k) {
    NrmGridLayout L;
    const size_t ts = elem_size(dtype), P = (size_t)ball_slots(m);
    size_t off = 0;
    L.plans = off;   off = up256(off + (size_t)N * BALL_PLAN_BYTES);
    L.keys = off;    off = up256(off + (size_t)N * P * 8);
    L.perm = off;    off = up256(off + (size_t)N * P * 4);
    L.rows4 = off;   off = up256(off + (size_t)N * P * 4 * ts);
    L.nbr_s = off;   off = up256(off + (size_t)N * P * k * 4);
    L.total = off;
    return L;
}

// ------------------------------------------------------------------ the two layouts of the fit and the backward
// GRID = false: the x-sorted cloud (row stride m_pad, tgs4 / tperm, live = s < rows[b], every list k_eff = min(k, rows[b]) long);
// GRID = true: the cell grid (row stride P, rows4 / perm, live = s < the plan's cnt, a list as long as its filled entries)
template <typename T, bool GRID>
__device__ __forceinline__ int nrm_live_rows(const int32_t* __restrict__ rows, const void* __restrict__ plans, int b, int m) {
    if constexpr (GRID) return min(plan_of<T>(plans, b).cnt, m);
    else return rows_of(rows, b, m);
}
template <bool GRID>
__device__ __forceinline__ int nrm_k_eff(const int32_t* __restrict__ nb, int k, int mb) {
    if constexpr (GRID) {
        int n = 0;
        for (int o = 0; o < k; ++o) n += nb[o] >= 0;    // (the filled entries lead the list)
        return n;
    } else return min(k, mb);
}

// ------------------------------------------------------------------ per-point eigen-system (forward and backward)
struct NrmPoint {
    double mu[3], lam[3], v[9], s;
    int k_eff;
};
template <typename T>
__device__ __forceinline__ void nrm_point(const typename V4<T>::type* __restrict__ rows4, const int32_t* __restrict__ nb, int k_eff,
                                          const typename V4<T>::type& p, const T* __restrict__ vp, NrmPoint& P) {
    P.k_eff = k_eff;
    double sum[3] = {0.0, 0.0, 0.0};
    for (int o = 0; o < k_eff; ++o) {
        const auto y = rows4[max(nb[o], 0)];      // (-1 only in the walk's lists, next to rows whose d2 overflows: output unspecified there)
        sum[0] += (double)y.x - (double)p.x; sum[1] += (double)y.y - (double)p.y; sum[2] += (double)y.z - (double)p.z;
    }
    P.mu[0] = sum[0] / k_eff; P.mu[1] = sum[1] / k_eff; P.mu[2] = sum[2] / k_eff;
    double C6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int o = 0; o < k_eff; ++o) {
        const auto y = rows4[max(nb[o], 0)];      // (-1 only in the walk's lists, next to rows whose d2 overflows: output unspecified there)
        const double dd[3] = {((double)y.x - (double)p.x) - P.mu[0], ((double)y.y - (double)p.y) - P.mu[1], ((double)y.z - (double)p.z) - P.mu[2]};
        nrm_cov_add(C6, dd);
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) C6[e] /= k_eff;
    nrm_eig(C6, P.lam, P.v);
    const double dv[3] = {(vp ? (double)vp[0] : 0.0) - (double)p.x, (vp ? (double)vp[1] : 0.0) - (double)p.y, (vp ? (double)vp[2] : 0.0) - (double)p.z};
    P.s = nrm_sign(P.v, dv);
}

inline int nrm_check(int dtype, int N, int m, int k, int vp_per_cloud) {
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (N <= 0 || m <= 0 || k < 3 || k > NRM_KMAX || (vp_per_cloud != 0 && vp_per_cloud != 1)) return DICP_ERR_SHAPE;
    if ((size_t)dicp_padded_targets(m) > 0x7fffffffu / NRM_KMAX) return DICP_ERR_SHAPE;
    return 0;
}

inline int nrm_grid_check(int dtype, int N, int m, int k, int c, int vp_per_cloud) {
    int rc = nrm_check(dtype, N, m, k, vp_per_cloud);
    if (rc || (rc = ball_check(dtype, N, m))) return rc;
    if (c < 3 || (size_t)ball_slots(m) > 0x7fffffffu / NRM_KMAX) return DICP_ERR_SHAPE;
    return 0;
}

}  // namespace
