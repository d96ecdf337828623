// Whole-ball surface normals for batches of clouds, forward and backward (dicp_amd/normals.py: estimate_normals_ball).  The rules are
// csrc/dicp_normals_ball.h's, the member list, its order and the coverage proof of the walk csrc/dicp_iss_ball.h's; the grid is the one
// dicp_ball_grid_build makes (csrc/ball_query.hip), read here and never built.  No index and no d2 tensor is written or read.  Everything
// is in double with no float atomics and nothing read back: all three passes are bit-reproducible and equal tests/normals_ball_ref.py bit
// for bit.
//
// The layout is iss_ball.hip's: one lane per SORTED SLOT of the grid (P = 2^ceil(log2 m) per cloud), one wave per workgroup, the outputs
// scattered to the original row perm[slot]; a lane whose perm is below m stores its row's element of every output -- zeros for a row
// outside the grid --, the padding lanes of the sort store no output.  So every element is stored exactly once and nothing is zero-filled.
// Forward (dicp_normals_ball_forward): the two walks of the ISS pass (sum and count; then the six sums), the Jacobi sweeps with the
//   rotations also applied to V, the sign, and the state of dicp_normals_ball.h (C6, mu, n, s: NBL_STATE doubles a slot, element-major so
//   that a wave's stores are consecutive) to the workspace the autograd context keeps.
// Records (dicp_normals_ball_records): no walk.  State + cotangents -> the 13 doubles of every slot, IN SORTED-SLOT ORDER: the gather reads
//   the record of slot j right beside rows4[j].  The eigen-system is recomputed from the stored C6 by the forward's own statements (12
//   doubles less of state than storing lam and V).  Every slot of the cloud gets a record, f = 0 for the rows outside the grid and the padding.
// Gather (dicp_normals_ball_gather): one walk; per member one 104-byte record.  Every element of the (N, m, c) gradient is stored once,
//   the zeros of the rows outside the grid and of the columns >= 3 included.
// `visited` (optional, for scripts/normals_ball_bench.py and the tests): the rows visited per cloud, added to the caller's zeroed counters
//   with integer atomics, one per lane -- a diagnostic that touches no output.
// No spin-waits, no cooperative launch; every loop is bounded by the cloud's row count (iss_ball_scan's bound).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_normals_ball.h"
#include "kernels_grid_plan.h"

namespace {

template <typename T>
__global__ __launch_bounds__(WAVE) void normals_ball_forward_kernel(const void* __restrict__ plans, const uint64_t* __restrict__ keys,
                                                                    const int32_t* __restrict__ perm, const typename V4<T>::type* __restrict__ rows4,
                                                                    int m, int Pm, int bpc, double radius, int min_neighbors,
                                                                    const T* __restrict__ viewpoint, int vp_per_cloud, double* __restrict__ state_ws,
                                                                    T* __restrict__ nrm_out, T* __restrict__ curv_out, T* __restrict__ eig_out,
                                                                    int32_t* __restrict__ count_out, unsigned long long* __restrict__ visited_out) {
    using T4 = typename V4<T>::type;
    const int b = blockIdx.x / bpc, s = (blockIdx.x - b * bpc) * WAVE + threadIdx.x;
    if (s >= Pm) return;
    const size_t gbase = (size_t)b * Pm;
    const int i = perm[gbase + s];
    if (i < 0 || i >= m) return;                                        // the padding of the sort: no row of the outputs
    BallPlan<T> pl = plan_of<T>(plans, b);
    pl.cnt = min(max(pl.cnt, 0), m);                                    // (the grid's own count: the clamp is a belt for the loads below)
    double l[3] = {0.0, 0.0, 0.0}, n3[3] = {0.0, 0.0, 0.0}, curv = 0.0;
    int count = 0;
    if (s < pl.cnt) {                                                   // the live rows are the first cnt sorted slots
        const uint64_t* kb = keys + gbase;
        auto key = [&](int j) -> uint64_t { return kb[j]; };
        auto row = [&](int j) -> T4 { return rows4[gbase + j]; };
        const T* v = viewpoint ? viewpoint + (vp_per_cloud ? (size_t)b * 3 : 0) : nullptr;
        const double vp[3] = {v ? (double)v[0] : 0.0, v ? (double)v[1] : 0.0, v ? (double)v[2] : 0.0};
        double st[NBL_STATE];
        unsigned visited;
        nbl_forward_row<T>(pl, iss_ball_R<T>(radius), radius * radius, s, key, row, vp, min_neighbors, l, n3, curv, st, count, visited);
        double* sw = state_ws + gbase * NBL_STATE + s;
#pragma unroll
        for (int e = 0; e < NBL_STATE; ++e) sw[(size_t)e * Pm] = st[e];
        if (visited_out) atomicAdd(visited_out + b, (unsigned long long)visited);            // diagnostics only: an integer count
    }
    const size_t o = (size_t)b * m + i;
    T* no = nrm_out + o * 3;
    no[0] = (T)n3[0]; no[1] = (T)n3[1]; no[2] = (T)n3[2];
    if (curv_out) curv_out[o] = (T)curv;
    if (eig_out) {
        T* e = eig_out + o * 3;
        e[0] = (T)l[0]; e[1] = (T)l[1]; e[2] = (T)l[2];
    }
    if (count_out) count_out[o] = count;
}

template <typename T>
__global__ __launch_bounds__(WAVE) void normals_ball_records_kernel(const void* __restrict__ plans, const int32_t* __restrict__ perm,
                                                                    const typename V4<T>::type* __restrict__ rows4, int m, int Pm, int bpc,
                                                                    const T* __restrict__ g_nrm, const T* __restrict__ g_curv,
                                                                    const double* __restrict__ state_ws, double* __restrict__ records) {
    const int b = blockIdx.x / bpc, s = (blockIdx.x - b * bpc) * WAVE + threadIdx.x;
    if (s >= Pm) return;
    const size_t gbase = (size_t)b * Pm;
    const int i = perm[gbase + s];
    const int cnt = min(max(plan_of<T>(plans, b).cnt, 0), m);
    const bool live = s < cnt && i >= 0 && i < m;
    double st[NBL_STATE], p[3] = {0.0, 0.0, 0.0}, gn[3] = {0.0, 0.0, 0.0}, gk = 0.0;
#pragma unroll
    for (int e = 0; e < NBL_STATE; ++e) st[e] = 0.0;
    if (live) {
        const double* sw = state_ws + gbase * NBL_STATE + s;
#pragma unroll
        for (int e = 0; e < NBL_STATE; ++e) st[e] = sw[(size_t)e * Pm];
        iss_ball_load(rows4[gbase + s], p);
        const size_t o = (size_t)b * m + i;
        if (g_nrm) { gn[0] = (double)g_nrm[o * 3]; gn[1] = (double)g_nrm[o * 3 + 1]; gn[2] = (double)g_nrm[o * 3 + 2]; }
        if (g_curv) gk = (double)g_curv[o];
    }
    double R[NRM_REC];
    nbl_record(live, st, p, g_nrm != nullptr, gn, g_curv != nullptr, gk, sizeof(T) == 4 ? 1e-6 : 1e-12, R);
    double* out = records + (gbase + s) * NRM_REC;
#pragma unroll
    for (int e = 0; e < NRM_REC; ++e) out[e] = R[e];
}

template <typename T>
__global__ __launch_bounds__(WAVE) void normals_ball_gather_kernel(const void* __restrict__ plans, const uint64_t* __restrict__ keys,
                                                                   const int32_t* __restrict__ perm, const typename V4<T>::type* __restrict__ rows4,
                                                                   int m, int Pm, int bpc, int c, double radius, const double* __restrict__ records,
                                                                   T* __restrict__ grad, unsigned long long* __restrict__ visited_out) {
    using T4 = typename V4<T>::type;
    const int b = blockIdx.x / bpc, s = (blockIdx.x - b * bpc) * WAVE + threadIdx.x;
    if (s >= Pm) return;
    const size_t gbase = (size_t)b * Pm;
    const int i = perm[gbase + s];
    if (i < 0 || i >= m) return;                                        // the padding of the sort: no row of the gradient
    BallPlan<T> pl = plan_of<T>(plans, b);
    pl.cnt = min(max(pl.cnt, 0), m);
    double g[3] = {0.0, 0.0, 0.0};
    if (s < pl.cnt) {
        const uint64_t* kb = keys + gbase;
        const double* rb = records + gbase * NRM_REC;
        auto key = [&](int j) -> uint64_t { return kb[j]; };
        auto row = [&](int j) -> T4 { return rows4[gbase + j]; };
        auto rec = [&](int j) -> const double* { return rb + (size_t)j * NRM_REC; };
        unsigned visited;
        nbl_gather_row<T>(pl, iss_ball_R<T>(radius), radius * radius, s, key, row, rec, g, visited);
        if (visited_out) atomicAdd(visited_out + b, (unsigned long long)visited);
    }
    T* o = grad + ((size_t)b * m + i) * c;
    o[0] = (T)g[0]; o[1] = (T)g[1]; o[2] = (T)g[2];
    for (int e = 3; e < c; ++e) o[e] = T(0);
}

inline size_t state_bytes(int N, int m) { return up256((size_t)N * ball_slots(m) * NBL_STATE * sizeof(double)); }

// the checks of the three entry points after the null checks, in the order that decides the status of a bad call (iss_ball_check's)
int nbl_check(int dtype, int N, int m, double radius, int min_neighbors) {
    int rc = ball_check(dtype, N, m);
    if (rc) return rc;
    if ((size_t)N * (size_t)m >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;
    if ((size_t)N * (size_t)((ball_slots(m) + WAVE - 1) / WAVE) >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;
    if (min_neighbors < 3) return DICP_ERR_SHAPE;
    if (!(radius > 0.0 && radius < HUGE_VAL && radius * radius < HUGE_VAL)) return DICP_ERR_SHAPE;
    return 0;
}

}  // namespace

size_t dicp_normals_ball_workspace_bytes(int N, int m) {
    if (N <= 0 || m <= 0 || m > (1 << 30) || (size_t)N * (size_t)m >= ((size_t)1 << 31)) return 0;
    return state_bytes(N, m);
}

int dicp_normals_ball_forward(int dtype, const void* plans, const uint64_t* keys, const int32_t* perm, const void* rows4, int N, int m, double radius,
                              int min_neighbors, const void* viewpoint, int viewpoint_per_cloud, void* workspace, size_t workspace_bytes,
                              void* normals_out, void* curvature_out, void* eigenvalues_out, int32_t* count_out, unsigned long long* visited,
                              void* stream) {
    if (!plans || !keys || !perm || !rows4 || !workspace || !normals_out) return DICP_ERR_NULL;
    int rc = nbl_check(dtype, N, m, radius, min_neighbors);
    if (rc) return rc;
    if (workspace_bytes < state_bytes(N, m) || (viewpoint_per_cloud != 0 && viewpoint_per_cloud != 1)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(plans, 8) || misaligned(keys, 8) || misaligned(perm, 4) || misaligned(rows4, 4 * ts) ||
        misaligned(viewpoint, ts) || misaligned(normals_out, ts) || misaligned(curvature_out, ts) || misaligned(eigenvalues_out, ts) ||
        misaligned(count_out, 4) || misaligned(visited, 8))
        return DICP_ERR_ALIGN;
    const int Pm = ball_slots(m), bpc = (Pm + WAVE - 1) / WAVE;
    const unsigned g = (unsigned)N * (unsigned)bpc;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        normals_ball_forward_kernel<T><<<g, WAVE, 0, (hipStream_t)stream>>>(plans, keys, perm, (const typename V4<T>::type*)rows4, m, Pm, bpc, radius,
                                                                            min_neighbors, (const T*)viewpoint, viewpoint_per_cloud, (double*)workspace,
                                                                            (T*)normals_out, (T*)curvature_out, (T*)eigenvalues_out, count_out, visited);
    });
    return launch_status();
}

int dicp_normals_ball_records(int dtype, const void* plans, const int32_t* perm, const void* rows4, int N, int m, const void* g_normals,
                              const void* g_curvature, const void* workspace, size_t workspace_bytes, double* records, void* stream) {
    if (!plans || !perm || !rows4 || !workspace || !records) return DICP_ERR_NULL;
    int rc = nbl_check(dtype, N, m, 1.0, 3);                            // (no radius and no count here: the state holds what they decided)
    if (rc) return rc;
    if (workspace_bytes < state_bytes(N, m)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(plans, 8) || misaligned(perm, 4) || misaligned(rows4, 4 * ts) || misaligned(g_normals, ts) ||
        misaligned(g_curvature, ts) || misaligned(records, 8))
        return DICP_ERR_ALIGN;
    const int Pm = ball_slots(m), bpc = (Pm + WAVE - 1) / WAVE;
    const unsigned g = (unsigned)N * (unsigned)bpc;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        normals_ball_records_kernel<T><<<g, WAVE, 0, (hipStream_t)stream>>>(plans, perm, (const typename V4<T>::type*)rows4, m, Pm, bpc, (const T*)g_normals,
                                                                            (const T*)g_curvature, (const double*)workspace, records);
    });
    return launch_status();
}

int dicp_normals_ball_gather(int dtype, const void* plans, const uint64_t* keys, const int32_t* perm, const void* rows4, int N, int m, int c,
                             double radius, const double* records, void* grad_out, unsigned long long* visited, void* stream) {
    if (!plans || !keys || !perm || !rows4 || !records || !grad_out) return DICP_ERR_NULL;
    int rc = nbl_check(dtype, N, m, radius, 3);
    if (rc) return rc;
    if (c < 3 || (size_t)N * (size_t)m * (size_t)c >= ((size_t)1 << 40)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(plans, 8) || misaligned(keys, 8) || misaligned(perm, 4) || misaligned(rows4, 4 * ts) || misaligned(records, 8) ||
        misaligned(grad_out, ts) || misaligned(visited, 8))
        return DICP_ERR_ALIGN;
    const int Pm = ball_slots(m), bpc = (Pm + WAVE - 1) / WAVE;
    const unsigned g = (unsigned)N * (unsigned)bpc;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        normals_ball_gather_kernel<T><<<g, WAVE, 0, (hipStream_t)stream>>>(plans, keys, perm, (const typename V4<T>::type*)rows4, m, Pm, bpc, c, radius,
                                                                           records, (T*)grad_out, visited);
    });
    return launch_status();
}
