// Exact k nearest neighbours on a sorted cell grid (dicp_amd/knn.py: knn_points / chamfer_distance with method="grid").  The plan, the
// stopping rule with its proof and the per-query scan are csrc/dicp_gridknn.h; this file is the device structure around them.
//
// The grid of a cloud (dicp_knn_grid_build) is ball_query's (csrc/kernels_grid.h: keys, bitonic sort, pack), with one difference: the
// plan kernel takes the cell edge from the cloud's own density (gknn_plan) instead of a radius (gknn_grid_build, kernels_grid.h).  The layout of plans / keys / perm /
// rows4 is dicp_ball_grid_build's, so the queries are ordered by dicp_ball_grid_build(order_by = these plans) and the backward is
// dicp_ball_query_backward, both unchanged.
// Search (dicp_knn_grid_query), one lane per sorted query slot: gknn_scan with the keys, rows and permutation read from global memory
// (L2: the lanes of a wave are neighbours in the grid and read the same lines), the list code and the capacities K of knn_points.
// Outputs in the original query order: d2, idx, and the sorted slot of every entry in the workspace.  Every loop is bounded by the
// cloud's row count and T's exponent range (dicp_gridknn.h).  No float atomics, nothing read back, every launch capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_fill.h"
#include "dicp_gridknn.h"
#include "kernels_grid.h"

namespace {

template <typename T, int K>
__global__ __launch_bounds__(BLOCK) void gknn_query_kernel(const T* __restrict__ x, int cx, int n, int Pn, const uint64_t* __restrict__ xkeys,
                                                           const int32_t* __restrict__ xperm, const void* __restrict__ plans,
                                                           const uint64_t* __restrict__ ykeys, const int32_t* __restrict__ yperm,
                                                           const typename V4<T>::type* __restrict__ yrows4, int Pm, int N, int k, int bpc,
                                                           T* __restrict__ d2_out, int64_t* __restrict__ idx_out, int32_t* __restrict__ slots,
                                                           unsigned long long* __restrict__ visited, unsigned long long* __restrict__ passes) {
    using T4 = typename V4<T>::type;
    int b, blk;
    if (!decode_block(bpc, N, b, blk)) return;
    const int s = blk * BLOCK + threadIdx.x;
    unsigned long long steps = 0, boxes = 0;
    if (s < n) {                                            // the first n sorted slots are the n query rows
        const size_t xs = (size_t)b * Pn + s;
        const int q = min(max(xperm[xs], 0), n - 1);
        const bool live = xkeys[xs] != BALL_NO_KEY;
        const size_t ybase = (size_t)b * Pm;
        T d[K];
        int id[K], sl[K];
        topk_init(d, id, sl, k);
        if (live) {
            const BallPlan<T> pl = plan_of<T>(plans, b);
            const T* xp = x + ((size_t)b * n + q) * cx;
            T4 p = {};
            p.x = xp[0]; p.y = xp[1]; p.z = xp[2];
            const uint64_t* kb = ykeys + ybase;
            auto keys = [&](int j) -> uint64_t { return kb[j]; };
            auto row = [&](int j) -> T4 { return yrows4[ybase + j]; };
            auto orig = [&](int j) -> int { return yperm[ybase + j]; };
            const auto ins = topk_inserter(d, id, sl, orig);
            const GknnScan r = gknn_scan<T>(pl, d, p, keys, row, ins);
            steps = r.visited;
            boxes = (unsigned long long)r.passes;
        }
        const size_t o0 = ((size_t)b * n + q) * k;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            if (i < K - k) continue;
            const int o = i - (K - k);
            d2_out[o0 + o] = d[i];
            idx_out[o0 + o] = id[i];
            slots[o0 + o] = sl[i];
        }
    }
    if (visited) wave_add(visited + b, steps);          // diagnostics: rows fed and passes made, one atomic per wave each
    if (passes) wave_add(passes + b, boxes);
}

}  // namespace

int dicp_knn_grid_build(int dtype, const void* pts, int c, const int32_t* rows, int N, int m, void* plans, uint64_t* keys, int32_t* perm,
                        void* rows4, void* stream) {
    if (!pts || !plans || !keys || !perm || !rows4) return DICP_ERR_NULL;
    int rc = ball_check(dtype, N, m);
    if (rc) return rc;
    if (c < 3) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(pts, ts) || misaligned(rows, 4) || misaligned(plans, 8) || misaligned(keys, 8) || misaligned(perm, 4) || misaligned(rows4, 4 * ts)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    begin_launch();
    rc = dtype == DICP_F32 ? gknn_grid_build<float>((const float*)pts, c, rows, N, m, plans, keys, perm, rows4, st)
                           : gknn_grid_build<double>((const double*)pts, c, rows, N, m, plans, keys, perm, rows4, st);
    if (rc) return rc;
    return launch_status();
}

int dicp_knn_grid_query(int dtype, const void* x, int cx, int n, const uint64_t* x_keys, const int32_t* x_perm, const void* y_plans,
                        const uint64_t* y_keys, const int32_t* y_perm, const void* y_rows4, int m, int N, int k,
                        void* d2, int64_t* idx, void* workspace, size_t workspace_bytes, unsigned long long* visited, unsigned long long* passes,
                        void* stream) {
    int rc = grid_query_check(dtype, x, cx, n, x_keys, x_perm, y_plans, y_keys, y_perm, y_rows4, m, N, k, d2, idx, workspace, workspace_bytes, visited);
    if (rc) return rc;
    if (misaligned(passes, 8)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (visited && (rc = dicp_fill::zero(visited, (size_t)N * sizeof(unsigned long long), st))) return rc;
    if (passes && (rc = dicp_fill::zero(passes, (size_t)N * sizeof(unsigned long long), st))) return rc;
    const int Pn = ball_slots(n), Pm = ball_slots(m);
    const int bpc = (n + BLOCK - 1) / BLOCK;
    const unsigned g = grid_for(N, bpc);
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        topk_with_kcap(k, [&](auto kcap) {
            gknn_query_kernel<T, decltype(kcap)::value><<<g, BLOCK, 0, st>>>((const T*)x, cx, n, Pn, x_keys, x_perm, y_plans, y_keys, y_perm,
                (const typename V4<T>::type*)y_rows4, Pm, N, k, bpc, (T*)d2, idx, (int32_t*)workspace, visited, passes);
        });
    });
    return launch_status();
}
