// Fixed-radius neighbours on a sorted cell grid (dicp_amd/ball.py: ball_query).  The arithmetic, the exactness proof and the per-query
// scan are csrc/dicp_ball.h; this file is the device structure around them.
//
// The grid of a cloud (dicp_ball_grid_build, order_by = NULL), O(m) memory whatever extent / radius is -- no table of cells:
// (the kernels of these stages but the plan's are csrc/kernels_grid.h, shared with knn_grid.hip)
//   plan    ball_plan_kernel, one workgroup per cloud: the bounds and the number of the live rows (j < rows[b], three finite coordinates),
//           then one lane runs ball_plan: origin, search half-width R, cell edges (enlarged until the key fits), key widths.  The host never
//           learns any of them; the radius itself is read from device memory.
//   keys    ball_keys_kernel: the 64-bit cell key of every live row, BALL_NO_KEY for the others and for the padding to P = 2^ceil(log2 m).
//   sort    a bitonic sort of (key, row index) pairs, P per cloud: ball_sort_local sorts chunks of up to 2048 pairs in LDS (every stage
//           with a stride inside the chunk), ball_sort_global does one stage with a larger stride.  1 + sum_{P' = 4096 .. P} (log2(P' / 2048)
//           + 1) launches: 10 for 16384 rows.  The pairs are distinct, so the result does not depend on the network: live rows by (key,
//           index), then the others by index.
//   pack    ball_pack_kernel: the live rows as (x, y, z, 0) in sorted order.
// The queries are ordered by the same kernels (order_by = the grid's plans): their key is that of the nearest grid cell, so that the lanes
// of a wave visit the same cells; the first n sorted slots are exactly the n query rows, the ones without neighbours (past x_rows[b], or
// with a non-finite coordinate) last.
// Search (dicp_ball_query), one lane per sorted query slot: ball_scan of dicp_ball.h with the keys, rows and permutation read from global
// memory (a cloud of 16384 rows is 128 KiB of keys and 256 KiB of rows: L2, and the lanes of a wave read the same lines), the list code
// and the capacities K of knn_points.  Outputs in the original query order: d2, idx, counts, and the sorted slot of every entry in the
// workspace for the backward.  Every loop is bounded by the cloud's row count (dicp_ball.h).  No float atomics: bit-reproducible.
// Backward (dicp_ball_query_backward), one lane per query: the 2 g (x - y) terms in double, the x-gradient summed in list order and written
// once, the y-gradient added to the original rows with float atomics after a zero-fill kernel (not bit-reproducible from run to run).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_fill.h"
#include "dicp_ball.h"
#include "kernels_grid.h"

namespace {

template <typename T>
__global__ __launch_bounds__(BLOCK) void ball_plan_kernel(const T* __restrict__ pts, int c, const int32_t* __restrict__ rows, int m,
                                                          const T* __restrict__ radius, void* __restrict__ plans) {
    T mn[3], mx[3];
    int cnt;
    ball_cloud_bounds<T>(pts, c, rows, m, mn, mx, cnt);
    if (threadIdx.x == 0) *(BallPlan<T>*)((char*)plans + (size_t)blockIdx.x * BALL_PLAN_BYTES) = ball_plan<T>(mn, mx, cnt, radius[0]);
}

template <typename T, int K>
__global__ __launch_bounds__(BLOCK) void ball_query_kernel(const T* __restrict__ x, int cx, int n, int Pn, const uint64_t* __restrict__ xkeys,
                                                           const int32_t* __restrict__ xperm, const void* __restrict__ plans,
                                                           const uint64_t* __restrict__ ykeys, const int32_t* __restrict__ yperm,
                                                           const typename V4<T>::type* __restrict__ yrows4, int m, int Pm, int N, int k, int bpc,
                                                           T* __restrict__ d2_out, int64_t* __restrict__ idx_out, int32_t* __restrict__ counts,
                                                           int32_t* __restrict__ slots, unsigned long long* __restrict__ visited) {
    using T4 = typename V4<T>::type;
    int b, blk;
    if (!decode_block(bpc, N, b, blk)) return;
    const int s = blk * BLOCK + threadIdx.x;
    unsigned long long steps = 0;
    if (s < n) {                                            // the first n sorted slots are the n query rows
        const size_t xs = (size_t)b * Pn + s;
        const int q = min(max(xperm[xs], 0), n - 1);
        const bool live = xkeys[xs] != BALL_NO_KEY;
        const size_t ybase = (size_t)b * Pm;
        T d[K];
        int id[K], sl[K];
        topk_init(d, id, sl, k);
        int count = 0;
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
            const BallScan r = ball_scan<T>(pl, p, keys, row, ins);
            count = r.count;
            steps = r.visited;
        }
        const size_t o0 = ((size_t)b * n + q) * k;
        counts[(size_t)b * n + q] = count;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            if (i < K - k) continue;
            const int o = i - (K - k);
            d2_out[o0 + o] = d[i];
            idx_out[o0 + o] = id[i];
            slots[o0 + o] = sl[i];
        }
    }
    if (visited) wave_add(visited + b, steps);          // diagnostics: rows visited, one atomic per wave
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void ball_bwd_kernel(const T* __restrict__ g_d2, const T* __restrict__ x, int cx, int n,
                                                         const typename V4<T>::type* __restrict__ yrows4, const int32_t* __restrict__ yperm,
                                                         int m, int Pm, int cy, int N, int k, int bpc, const int32_t* __restrict__ slots,
                                                         T* __restrict__ grad_x, T* __restrict__ grad_y) {
    int b, blk;
    if (!decode_block(bpc, N, b, blk)) return;
    const int i = blk * BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t row = (size_t)b * n + i, ybase = (size_t)b * Pm;
    const T* xp = x + row * cx;
    const T* g = g_d2 + row * k;
    const int32_t* sl = slots + row * k;
    double gx[3] = {0.0, 0.0, 0.0};
    for (int o = 0; o < k; ++o) {
        const int j = sl[o];
        if (j < 0 || j >= Pm) continue;
        const double f = 2.0 * (double)g[o];
        if (f == 0.0) continue;
        const auto y = yrows4[ybase + j];
        const double e[3] = {(double)xp[0] - (double)y.x, (double)xp[1] - (double)y.y, (double)xp[2] - (double)y.z};
        gx[0] += f * e[0]; gx[1] += f * e[1]; gx[2] += f * e[2];
        if (grad_y) {
            const int l = yperm[ybase + j];
            if (l >= 0 && l < m) {
                T* a = grad_y + ((size_t)b * m + l) * cy;
                unsafeAtomicAdd(a, (T)(-f * e[0])); unsafeAtomicAdd(a + 1, (T)(-f * e[1])); unsafeAtomicAdd(a + 2, (T)(-f * e[2]));
            }
        }
    }
    if (grad_x) {
        T* r = grad_x + row * cx;
        r[0] = (T)gx[0]; r[1] = (T)gx[1]; r[2] = (T)gx[2];
        for (int a = 3; a < cx; ++a) r[a] = T(0);
    }
}

}  // namespace

int dicp_ball_grid_slots(int m) { return m > 0 && m <= (1 << 30) ? ball_slots(m) : 0; }
int dicp_ball_plan_bytes(void) { return BALL_PLAN_BYTES; }

int dicp_ball_grid_build(int dtype, const void* pts, int c, const int32_t* rows, int N, int m, const void* radius, const void* order_by,
                         void* plans, uint64_t* keys, int32_t* perm, void* rows4, void* stream) {
    if (!pts || !keys || !perm) return DICP_ERR_NULL;
    if (order_by ? (plans || rows4) : (!plans || !rows4 || !radius)) return DICP_ERR_NULL;
    int rc = ball_check(dtype, N, m);
    if (rc) return rc;
    if (c < 3) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(pts, ts) || misaligned(rows, 4) || misaligned(radius, ts) || misaligned(order_by, 8) || misaligned(plans, 8) || misaligned(keys, 8) ||
        misaligned(perm, 4) || misaligned(rows4, 4 * ts)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const void* pl = order_by ? order_by : plans;
    begin_launch();
    rc = with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        if (!order_by) ball_plan_kernel<T><<<N, BLOCK, 0, st>>>((const T*)pts, c, rows, m, (const T*)radius, plans);
        return ball_grid_stages<T>((const T*)pts, c, rows, N, m, pl, order_by ? 0 : 1, keys, perm, rows4, st);
    });
    if (rc) return rc;
    return launch_status();
}

size_t dicp_ball_query_workspace_bytes(int dtype, int N, int n, int k) {
    if (ball_check(dtype, N, n) || k < 1 || k > BALL_KMAX) return 0;
    return up256((size_t)N * n * k * 4);
}

int dicp_ball_query(int dtype, const void* x, int cx, int n, const uint64_t* x_keys, const int32_t* x_perm, const void* y_plans,
                    const uint64_t* y_keys, const int32_t* y_perm, const void* y_rows4, int m, int N, int k,
                    void* d2, int64_t* idx, int32_t* counts, void* workspace, size_t workspace_bytes, unsigned long long* visited, void* stream) {
    if (!counts) return DICP_ERR_NULL;
    int rc = grid_query_check(dtype, x, cx, n, x_keys, x_perm, y_plans, y_keys, y_perm, y_rows4, m, N, k, d2, idx, workspace, workspace_bytes, visited);
    if (rc) return rc;
    if (misaligned(counts, 4)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (visited && (rc = dicp_fill::zero(visited, (size_t)N * sizeof(unsigned long long), st))) return rc;
    const int Pn = ball_slots(n), Pm = ball_slots(m);
    const int bpc = (n + BLOCK - 1) / BLOCK;
    const unsigned g = grid_for(N, bpc);
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        topk_with_kcap(k, [&](auto kcap) {
            ball_query_kernel<T, decltype(kcap)::value><<<g, BLOCK, 0, st>>>((const T*)x, cx, n, Pn, x_keys, x_perm, y_plans, y_keys, y_perm,
                (const typename V4<T>::type*)y_rows4, m, Pm, N, k, bpc, (T*)d2, idx, counts, (int32_t*)workspace, visited);
        });
    });
    return launch_status();
}

int dicp_ball_query_backward(int dtype, const void* g_d2, const void* x, int cx, int n, const void* y_rows4, const int32_t* y_perm, int m, int cy,
                             int N, int k, const void* fwd_workspace, void* grad_x, void* grad_y, void* stream) {
    if (!g_d2 || !x || !y_rows4 || !y_perm || !fwd_workspace) return DICP_ERR_NULL;
    int rc = ball_check(dtype, N, n);
    if (rc || (rc = ball_check(dtype, N, m))) return rc;
    if (cx < 3 || cy < 3 || k < 1 || k > BALL_KMAX) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(g_d2, ts) || misaligned(x, ts) || misaligned(y_rows4, 4 * ts) || misaligned(y_perm, 4) || misaligned(fwd_workspace, 4) ||
        misaligned(grad_x, ts) || misaligned(grad_y, ts)) return DICP_ERR_ALIGN;
    if (!grad_x && !grad_y) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (grad_y && (rc = dicp_fill::zero(grad_y, (size_t)N * m * cy * ts, st))) return rc;
    const int Pm = ball_slots(m);
    const int bpc = (n + BLOCK - 1) / BLOCK;
    const unsigned g = grid_for(N, bpc);
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        ball_bwd_kernel<T><<<g, BLOCK, 0, st>>>((const T*)g_d2, (const T*)x, cx, n, (const typename V4<T>::type*)y_rows4, y_perm, m, Pm, cy,
            N, k, bpc, (const int32_t*)fwd_workspace, (T*)grad_x, (T*)grad_y);
    });
    return launch_status();
}
