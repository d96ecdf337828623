// The device structure of a cloud's cell grid, shared by csrc/ball_query.hip (fixed-radius neighbours) and csrc/knn_grid.hip (k nearest
// neighbours): the bounds of a cloud's live rows for the plan kernels, the keys, the bitonic sort of (key, row) pairs and the pack of the
// sorted rows; and the whole build of a density grid (the plan of csrc/dicp_gridknn.h, then those stages), shared by csrc/knn_grid.hip and
// csrc/normals.hip (estimate_normals with method="grid").  What the stages are for is told at the top of ball_query.hip; the arithmetic
// is csrc/dicp_ball.h.
// Everything here has internal linkage (anonymous namespace): each .hip file gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_ball.h"
#include "dicp_gridknn.h"
#include "kernels_grid_plan.h"

namespace {

constexpr int BALL_KMAX = 32;
constexpr int BALL_CHUNK = 2048;                        // pairs a workgroup sorts in LDS: 24 KiB

// The per-axis bounds mn / mx and the number cnt of the live rows (j < rows[b], three finite coordinates) of cloud b = blockIdx.x, one
// workgroup of BLOCK threads per cloud; the result is thread 0's (the others hold partial values)
template <typename T>
__device__ __forceinline__ void ball_cloud_bounds(const T* __restrict__ pts, int c, const int32_t* __restrict__ rows, int m, T* mn, T* mx, int& cnt) {
    __shared__ T smn[3][BLOCK / WAVE], smx[3][BLOCK / WAVE];
    __shared__ int scnt[BLOCK / WAVE];
    const int b = blockIdx.x;
    const int mb = rows_of(rows, b, m);
    const T* base = pts + (size_t)b * m * c;
    for (int d = 0; d < 3; ++d) { mn[d] = inf_v<T>(); mx[d] = -inf_v<T>(); }
    cnt = 0;
    for (int j = threadIdx.x; j < mb; j += BLOCK) {
        const T* p = base + (size_t)j * c;
        const T x = p[0], y = p[1], z = p[2];
        if (ball_finite(x) && ball_finite(y) && ball_finite(z)) {
            ++cnt;
            mn[0] = min_t(mn[0], x); mn[1] = min_t(mn[1], y); mn[2] = min_t(mn[2], z);
            mx[0] = max_t(mx[0], x); mx[1] = max_t(mx[1], y); mx[2] = max_t(mx[2], z);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_xor(cnt, off);
#pragma unroll
        for (int d = 0; d < 3; ++d) { mn[d] = min_t(mn[d], __shfl_xor(mn[d], off)); mx[d] = max_t(mx[d], __shfl_xor(mx[d], off)); }
    }
    const int w = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        scnt[w] = cnt;
        for (int d = 0; d < 3; ++d) { smn[d][w] = mn[d]; smx[d][w] = mx[d]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < BLOCK / WAVE; ++i) {
            cnt += scnt[i];
            for (int d = 0; d < 3; ++d) { mn[d] = min_t(mn[d], smn[d][i]); mx[d] = max_t(mx[d], smx[d][i]); }
        }
    }
}

// key / idx (N,P): the pairs to sort.  own = 1: the rows of the grid's own cloud; 0: the queries of another cloud
template <typename T>
__global__ __launch_bounds__(BLOCK) void ball_keys_kernel(const T* __restrict__ pts, int c, const int32_t* __restrict__ rows, int N, int m, int P,
                                                          const void* __restrict__ plans, int own, uint64_t* __restrict__ key, int32_t* __restrict__ idx) {
    const size_t total = (size_t)N * P;
    for (size_t e = (size_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (size_t)gridDim.x * BLOCK) {
        const int b = (int)(e / P), j = (int)(e - (size_t)b * P);
        uint64_t k = BALL_NO_KEY;
        if (j < rows_of(rows, b, m)) {
            const BallPlan<T>& pl = plan_of<T>(plans, b);
            const T* p = pts + ((size_t)b * m + j) * c;
            const T x = p[0], y = p[1], z = p[2];
            if (ball_finite(x) && ball_finite(y) && ball_finite(z) && (!own || pl.cnt > 0)) k = ball_point_key(pl, x, y, z);
        }
        key[e] = k;
        idx[e] = j;
    }
}

__device__ __forceinline__ bool pair_after(uint64_t ka, int ia, uint64_t kb, int ib) { return ka > kb || (ka == kb && ia > ib); }

// Stages of the bitonic network on LDS-resident chunks of `chunk` pairs (a power of two <= BALL_CHUNK dividing P).
// k_from = 2: the whole network up to runs of `chunk` (k = 2 .. chunk); otherwise the strides chunk / 2 .. 1 of stage k = k_from.
__global__ __launch_bounds__(BLOCK) void ball_sort_local(uint64_t* __restrict__ key, int32_t* __restrict__ idx, int P, int chunk, int k_from, size_t chunks) {
    __shared__ uint64_t sk[BALL_CHUNK];
    __shared__ int32_t si[BALL_CHUNK];
    const size_t ch = blockIdx.x;
    if (ch >= chunks) return;
    const size_t base = ch * (size_t)chunk;
    const int i0 = (int)(base % (size_t)P);                 // the chunk's first position inside its cloud
    for (int t = threadIdx.x; t < chunk; t += BLOCK) { sk[t] = key[base + t]; si[t] = idx[base + t]; }
    __syncthreads();
    const int k_to = k_from == 2 ? chunk : k_from;
    for (int k = k_from; k <= k_to; k <<= 1) {
        for (int j = min(k, chunk) >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < chunk / 2; t += BLOCK) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const bool asc = ((i0 + i) & k) == 0;
                const uint64_t ka = sk[i], kb = sk[l];
                const int ia = si[i], ib = si[l];
                if (pair_after(ka, ia, kb, ib) == asc) { sk[i] = kb; sk[l] = ka; si[i] = ib; si[l] = ia; }
            }
            __syncthreads();
        }
    }
    for (int t = threadIdx.x; t < chunk; t += BLOCK) { key[base + t] = sk[t]; idx[base + t] = si[t]; }
}

// One stage (k, j) with j >= the chunk: N * P / 2 compare-exchanges in global memory
__global__ __launch_bounds__(BLOCK) void ball_sort_global(uint64_t* __restrict__ key, int32_t* __restrict__ idx, int P, int k, int j, size_t pairs) {
    const int half = P >> 1;
    for (size_t e = (size_t)blockIdx.x * BLOCK + threadIdx.x; e < pairs; e += (size_t)gridDim.x * BLOCK) {
        const size_t b = e / half;
        const int t = (int)(e - b * half);
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const bool asc = (i & k) == 0;
        uint64_t* kk = key + b * P;
        int32_t* ii = idx + b * P;
        const uint64_t ka = kk[i], kb = kk[l];
        const int ia = ii[i], ib = ii[l];
        if (pair_after(ka, ia, kb, ib) == asc) { kk[i] = kb; kk[l] = ka; ii[i] = ib; ii[l] = ia; }
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void ball_pack_kernel(const T* __restrict__ pts, int c, int N, int m, int P, const void* __restrict__ plans,
                                                          const int32_t* __restrict__ perm, typename V4<T>::type* __restrict__ rows4) {
    using T4 = typename V4<T>::type;
    const size_t total = (size_t)N * P;
    for (size_t e = (size_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (size_t)gridDim.x * BLOCK) {
        const int b = (int)(e / P), s = (int)(e - (size_t)b * P);
        T4 v = {};
        if (s < plan_of<T>(plans, b).cnt) {
            const int j = perm[e];
            if (j >= 0 && j < m) {
                const T* p = pts + ((size_t)b * m + j) * c;
                v.x = p[0]; v.y = p[1]; v.z = p[2];
            }
        }
        rows4[e] = v;
    }
}

// The arguments dicp_ball_query and dicp_knn_grid_query have in common, checked in the order that decides the status of a bad call
int grid_query_check(int dtype, const void* x, int cx, int n, const uint64_t* x_keys, const int32_t* x_perm, const void* y_plans,
                     const uint64_t* y_keys, const int32_t* y_perm, const void* y_rows4, int m, int N, int k, const void* d2, const int64_t* idx,
                     const void* workspace, size_t workspace_bytes, const unsigned long long* visited) {
    if (!x || !x_keys || !x_perm || !y_plans || !y_keys || !y_perm || !y_rows4 || !d2 || !idx || !workspace) return DICP_ERR_NULL;
    int rc = ball_check(dtype, N, n);
    if (rc || (rc = ball_check(dtype, N, m))) return rc;
    if (cx < 3 || k < 1 || k > BALL_KMAX || workspace_bytes < up256((size_t)N * n * k * 4)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(x, ts) || misaligned(x_keys, 8) || misaligned(x_perm, 4) || misaligned(y_plans, 8) || misaligned(y_keys, 8) || misaligned(y_perm, 4) ||
        misaligned(y_rows4, 4 * ts) || misaligned(d2, ts) || misaligned(idx, 8) || misaligned(workspace, 4) || misaligned(visited, 8)) return DICP_ERR_ALIGN;
    return 0;
}

int ball_sort(uint64_t* key, int32_t* idx, int N, int P, hipStream_t st) {
    const int chunk = P < BALL_CHUNK ? P : BALL_CHUNK;
    const size_t chunks = (size_t)N * (P / chunk), pairs = (size_t)N * (P / 2);
    if (chunks > 0x7fffffffu) return DICP_ERR_SHAPE;
    ball_sort_local<<<(unsigned)chunks, BLOCK, 0, st>>>(key, idx, P, chunk, 2, chunks);
    for (int k = chunk << 1; k <= P && k > 0; k <<= 1) {
        for (int j = k >> 1; j >= chunk; j >>= 1) ball_sort_global<<<grid_1d(pairs), BLOCK, 0, st>>>(key, idx, P, k, j, pairs);
        ball_sort_local<<<(unsigned)chunks, BLOCK, 0, st>>>(key, idx, P, chunk, k, chunks);
    }
    return 0;
}

// The stages after the plan: keys, sort and (own = 1, the grid's own cloud) pack.  pl: the plans the keys are taken with
template <typename T>
int ball_grid_stages(const T* pts, int c, const int32_t* rows, int N, int m, const void* pl, int own, uint64_t* keys, int32_t* perm, void* rows4, hipStream_t st) {
    const int P = ball_slots(m);
    const size_t total = (size_t)N * P;
    ball_keys_kernel<T><<<grid_1d(total), BLOCK, 0, st>>>(pts, c, rows, N, m, P, pl, own, keys, perm);
    const int rc = ball_sort(keys, perm, N, P, st);
    if (rc) return rc;
    if (own) ball_pack_kernel<T><<<grid_1d(total), BLOCK, 0, st>>>(pts, c, N, m, P, pl, perm, (typename V4<T>::type*)rows4);
    return 0;
}

// The density plan of every cloud (gknn_plan: the cell edge from the number and the bounds of the live rows), one workgroup per cloud
template <typename T>
__global__ __launch_bounds__(BLOCK) void gknn_plan_kernel(const T* __restrict__ pts, int c, const int32_t* __restrict__ rows, int m, void* __restrict__ plans) {
    T mn[3], mx[3];
    int cnt;
    ball_cloud_bounds<T>(pts, c, rows, m, mn, mx, cnt);
    if (threadIdx.x == 0) *(BallPlan<T>*)((char*)plans + (size_t)blockIdx.x * BALL_PLAN_BYTES) = gknn_plan<T>(mn, mx, cnt);
}

// The density grid of every cloud: plan, keys, sort, pack (the caller brackets it with begin_launch / launch_status)
template <typename T>
int gknn_grid_build(const T* pts, int c, const int32_t* rows, int N, int m, void* plans, uint64_t* keys, int32_t* perm, void* rows4, hipStream_t st) {
    gknn_plan_kernel<T><<<N, BLOCK, 0, st>>>(pts, c, rows, m, plans);
    return ball_grid_stages<T>(pts, c, rows, N, m, plans, 1, keys, perm, rows4, st);
}

}  // namespace
