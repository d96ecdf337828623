// k nearest neighbours between two clouds and the gradient of their squared distances (dicp_amd/knn.py: knn_points, chamfer_distance).
//
// Set-up (by the caller, once per cloud, through the existing entry points): dicp_sweep_sort + dicp_sweep_build with frame = NULL sort
// each cloud by raw x -- keys (N,m_pad) T, perm (N,m_pad) and the packed rows tgs4 (N,m_pad,4) T in sorted order.  Both clouds are
// sorted: the queries too, so that the 256 lanes of a block hold neighbouring x and walk overlapping target ranges.  chamfer_distance
// prepares each cloud once and searches it in both directions.
// Search (dicp_knn_points), one lane per sorted query slot:
//   start  the lower bound of the query's x among the target cloud's first y_rows[b] sorted keys: rows left of it have x < p.x, rows
//          from it on x >= p.x (NaN last).
//   walk   the two-cursor walk of csrc/dicp_topk.h from there, the side with the smaller gap first, stopping once gap^2 > the k-th best
//          d2.  The exactness argument of estimate_normals carries over unchanged: it never used that the query is a row of the cloud,
//          only that gap^2 is the xx of the row at the cursor -- fl(p.x - y.x) = -fl(y.x - p.x) exactly -- and that the gaps grow
//          outward from the split.  The block's target window (the span of its lanes' start positions +- WIN_HALO rows, capped at
//          WIN_ROWS) is staged in LDS; rows outside it are read from global memory.  The list capacity K is the smallest of
//          1, 4, 8, 16, 32 that holds k: chamfer's k = 1 compares once per row.  No float atomics: bit-reproducible.
//   out    d2 (N,n,k) T and idx (N,n,k) int64 in the original query order (+inf / -1 beyond k_eff and on query rows past x_rows[b]);
//          the sorted target slot of every entry (N,n_pad,k) int32 in the workspace, for the backward.
// Backward (dicp_knn_points_backward), one lane per sorted query slot: d d2 / dx_i = 2 (x_i - y_j), d d2 / dy_j = -2 (x_i - y_j), in
// double.  The x-gradient sums the lane's k entries in list order and is written once (bit-reproducible); the y-gradient goes into the
// sorted target slots through an LDS window spanning the slots the block uses (capped), global atomics outside it, and one
// dicp_permute_add_rows returns it to the original rows (float atomics: not bit-reproducible from run to run).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_fill.h"
#include "dicp_topk.h"

namespace {

constexpr int KNN_KMAX = 32;
template <typename T> struct WinHalo;                   // target rows staged on either side of the block's start span
template <> struct WinHalo<float>  { static constexpr int v = 1024; };
template <> struct WinHalo<double> { static constexpr int v = 512; };
template <typename T> struct WinRows;                   // at most this many: 36 KiB float4 / 40 KiB double4
template <> struct WinRows<float>  { static constexpr int v = BLOCK + 2 * 1024; };
template <> struct WinRows<double> { static constexpr int v = BLOCK + 2 * 512; };
template <typename T> struct BwdRows;                   // y-gradient window rows: 27 KiB float / 30 KiB double
template <> struct BwdRows<float>  { static constexpr int v = BLOCK + 2 * 1024; };
template <> struct BwdRows<double> { static constexpr int v = BLOCK + 2 * 512; };

template <typename T, int K>
__global__ __launch_bounds__(BLOCK) void knn_points_kernel(const typename V4<T>::type* __restrict__ xgs4, const int32_t* __restrict__ xperm,
                                                           const int32_t* __restrict__ x_rows, int n, int n_pad,
                                                           const T* __restrict__ ykeys, const typename V4<T>::type* __restrict__ ygs4,
                                                           const int32_t* __restrict__ yperm, const int32_t* __restrict__ y_rows, int m, int m_pad,
                                                           int N, int k, int bpc, T* __restrict__ d2_out, int64_t* __restrict__ idx_out,
                                                           int32_t* __restrict__ slots, unsigned long long* __restrict__ walked) {
    using T4 = typename V4<T>::type;
    constexpr int H = WinHalo<T>::v, W = WinRows<T>::v;
    __shared__ T4 win[W];
    __shared__ int span[2];
    int b, blk;
    if (!decode_block(bpc, N, b, blk)) return;
    const int nb = rows_of(x_rows, b, n), mb = rows_of(y_rows, b, m);
    const int s = blk * BLOCK + threadIdx.x;
    const size_t xbase = (size_t)b * n_pad, ybase = (size_t)b * m_pad;
    const bool live = s < nb;
    if (threadIdx.x == 0) { span[0] = 0x7fffffff; span[1] = -1; }
    __syncthreads();
    T4 p = {};
    int pos = 0;
    if (live) {
        p = xgs4[xbase + s];
        pos = topk_lower_bound(ykeys + ybase, mb, p.x);
        if (p.x == p.x) { atomicMin(&span[0], pos); atomicMax(&span[1], pos); }   // (a NaN query walks everything anyway)
    }
    __syncthreads();
    int wlo = 0, whi = 0;
    if (span[1] >= 0) {
        wlo = max(span[0] - H, 0);
        whi = min(min(span[1] + H, mb), wlo + W);
    }
    for (int r = threadIdx.x; r < whi - wlo; r += BLOCK) win[r] = ygs4[ybase + wlo + r];
    __syncthreads();
    unsigned long long steps = 0;
    if (live) {
        auto row = [&](int j) -> T4 { return (j >= wlo && j < whi) ? win[j - wlo] : ygs4[ybase + j]; };
        auto orig = [&](int j) -> int { return yperm[ybase + j]; };
        T d[K];
        int id[K], sl[K];
        topk_init(d, id, sl, k);
        const auto ins = topk_inserter(d, id, sl, orig);
        steps = topk_walk(d, p, pos - 1, pos, mb, row, ins);
        const size_t o0 = ((size_t)b * n + xperm[xbase + s]) * k;
        int32_t* so = slots + (xbase + s) * k;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            if (i < K - k) continue;
            const int o = i - (K - k);
            d2_out[o0 + o] = d[i];
            idx_out[o0 + o] = id[i];
            so[o] = sl[i];
        }
    } else if (s < n) {                                     // the query row s of the cloud's padding (original order)
        const size_t o0 = ((size_t)b * n + s) * k;
        for (int o = 0; o < k; ++o) { d2_out[o0 + o] = inf_v<T>(); idx_out[o0 + o] = -1; }
    }
    if (walked) wave_add(walked + b, steps);          // diagnostics: rows walked, one atomic per wave
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void knn_points_bwd_kernel(const T* __restrict__ g_d2, const typename V4<T>::type* __restrict__ xgs4,
                                                               const int32_t* __restrict__ xperm, const int32_t* __restrict__ x_rows, int n, int n_pad,
                                                               const typename V4<T>::type* __restrict__ ygs4, int m_pad, int N, int k, int bpc,
                                                               const int32_t* __restrict__ slots, T* __restrict__ grad_x, int cx,
                                                               T* __restrict__ gys /* (N,m_pad,3) sorted, or NULL */) {
    constexpr int W = BwdRows<T>::v;
    __shared__ T acc[W * 3];
    __shared__ int span[2];
    int b, blk;
    if (!decode_block(bpc, N, b, blk)) return;
    const int nb = rows_of(x_rows, b, n);
    const int s = blk * BLOCK + threadIdx.x;
    const size_t xbase = (size_t)b * n_pad, ybase = (size_t)b * m_pad;
    const bool live = s < nb;
    const int32_t* sl = slots + (xbase + s) * k;
    if (threadIdx.x == 0) { span[0] = 0x7fffffff; span[1] = -1; }
    __syncthreads();
    if (live && gys) {                                      // the window: the sorted target slots this block's lists use
        int lo = 0x7fffffff, hi = -1;
        for (int o = 0; o < k; ++o) {
            const int j = sl[o];
            if (j >= 0) { lo = min(lo, j); hi = max(hi, j); }
        }
        if (hi >= 0) { atomicMin(&span[0], lo); atomicMax(&span[1], hi); }
    }
    __syncthreads();
    const int wlo = span[1] >= 0 ? span[0] : 0, whi = span[1] >= 0 ? min(span[1] + 1, wlo + W) : 0, wn = (whi - wlo) * 3;
    for (int e = threadIdx.x; e < wn; e += BLOCK) acc[e] = T(0);
    __syncthreads();
    if (live) {
        const size_t orow = (size_t)b * n + xperm[xbase + s];
        const auto p = xgs4[xbase + s];
        const T* g = g_d2 + orow * k;
        double gx[3] = {0.0, 0.0, 0.0};
        for (int o = 0; o < k; ++o) {
            const int j = sl[o];
            if (j < 0) continue;
            const double f = 2.0 * (double)g[o];
            if (f == 0.0) continue;
            const auto y = ygs4[ybase + j];
            const double e[3] = {(double)p.x - (double)y.x, (double)p.y - (double)y.y, (double)p.z - (double)y.z};
            gx[0] += f * e[0]; gx[1] += f * e[1]; gx[2] += f * e[2];
            if (gys) {
                const T v0 = (T)(-f * e[0]), v1 = (T)(-f * e[1]), v2 = (T)(-f * e[2]);
                if (j >= wlo && j < whi) {
                    T* a = acc + (j - wlo) * 3;
                    atomicAdd(a, v0); atomicAdd(a + 1, v1); atomicAdd(a + 2, v2);
                } else {                                    // outside the window: the sorted rows directly
                    T* a = gys + (ybase + j) * 3;
                    unsafeAtomicAdd(a, v0); unsafeAtomicAdd(a + 1, v1); unsafeAtomicAdd(a + 2, v2);
                }
            }
        }
        if (grad_x) {
            T* r = grad_x + orow * cx;
            r[0] = (T)gx[0]; r[1] = (T)gx[1]; r[2] = (T)gx[2];
            for (int a = 3; a < cx; ++a) r[a] = T(0);
        }
    } else if (s < n && grad_x) {                           // the query row s of the cloud's padding: zero
        T* r = grad_x + ((size_t)b * n + s) * cx;
        for (int a = 0; a < cx; ++a) r[a] = T(0);
    }
    __syncthreads();
    T* out = gys ? gys + (ybase + wlo) * 3 : nullptr;       // the window: contiguous rows, which neighbouring blocks' windows overlap
    for (int e = threadIdx.x; e < wn; e += BLOCK) {
        const T v = acc[e];
        if (v != T(0)) unsafeAtomicAdd(out + e, v);
    }
}

int knn_check(int dtype, int N, int n, int m, int k) {
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (N <= 0 || n <= 0 || m <= 0 || k < 1 || k > KNN_KMAX) return DICP_ERR_SHAPE;
    if ((size_t)dicp_padded_targets(n) > 0x7fffffffu / KNN_KMAX) return DICP_ERR_SHAPE;
    return 0;
}

}  // namespace

size_t dicp_knn_points_workspace_bytes(int dtype, int N, int n, int m, int k, int backward) {
    if (knn_check(dtype, N, n, m, k)) return 0;
    const size_t ts = elem_size(dtype);
    if (backward) return up256((size_t)N * dicp_padded_targets(m) * 3 * ts);
    return up256((size_t)N * dicp_padded_targets(n) * k * 4);
}

int dicp_knn_points(int dtype, const void* x_tgs4, const int32_t* x_perm, const int32_t* x_rows, int n,
                    const void* y_keys, const void* y_tgs4, const int32_t* y_perm, const int32_t* y_rows, int m, int N, int k,
                    void* d2, int64_t* idx, void* workspace, size_t workspace_bytes, unsigned long long* walked, void* stream) {
    if (!x_tgs4 || !x_perm || !y_keys || !y_tgs4 || !y_perm || !d2 || !idx || !workspace) return DICP_ERR_NULL;
    int rc = knn_check(dtype, N, n, m, k);
    if (rc) return rc;
    if (workspace_bytes < dicp_knn_points_workspace_bytes(dtype, N, n, m, k, 0)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(x_tgs4, 4 * ts) || misaligned(y_tgs4, 4 * ts) || misaligned(y_keys, ts) || misaligned(x_perm, 4) || misaligned(y_perm, 4) ||
        misaligned(d2, ts) || misaligned(idx, 8) || misaligned(workspace, 4) || misaligned(x_rows, 4) || misaligned(y_rows, 4) ||
        misaligned(walked, 8)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (walked && (rc = dicp_fill::zero(walked, (size_t)N * sizeof(unsigned long long), st))) return rc;
    const int n_pad = dicp_padded_targets(n), m_pad = dicp_padded_targets(m);
    const int bpc = (n + BLOCK - 1) / BLOCK;
    const unsigned g = grid_for(N, bpc);
    int32_t* slots = (int32_t*)workspace;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        topk_with_kcap(k, [&](auto kcap) {
            knn_points_kernel<T, decltype(kcap)::value><<<g, BLOCK, 0, st>>>((const typename V4<T>::type*)x_tgs4, x_perm, x_rows, n, n_pad, (const T*)y_keys,
                (const typename V4<T>::type*)y_tgs4, y_perm, y_rows, m, m_pad, N, k, bpc, (T*)d2, idx, slots, walked);
        });
    });
    return launch_status();
}

int dicp_knn_points_backward(int dtype, const void* g_d2, const void* x_tgs4, const int32_t* x_perm, const int32_t* x_rows, int n, int cx,
                             const void* y_tgs4, const int32_t* y_perm, int m, int cy, int N, int k, const void* fwd_workspace,
                             void* grad_x, void* grad_y, void* workspace, size_t workspace_bytes, void* stream) {
    if (!g_d2 || !x_tgs4 || !x_perm || !y_tgs4 || !y_perm || !fwd_workspace) return DICP_ERR_NULL;
    if (grad_y && !workspace) return DICP_ERR_NULL;
    int rc = knn_check(dtype, N, n, m, k);
    if (rc) return rc;
    if (cx < 3 || cy < 3 || (grad_y && workspace_bytes < dicp_knn_points_workspace_bytes(dtype, N, n, m, k, 1))) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(g_d2, ts) || misaligned(x_tgs4, 4 * ts) || misaligned(y_tgs4, 4 * ts) || misaligned(x_perm, 4) || misaligned(y_perm, 4) ||
        misaligned(fwd_workspace, 4) || misaligned(x_rows, 4) || misaligned(grad_x, ts) || misaligned(grad_y, ts) || misaligned(workspace, 16)) return DICP_ERR_ALIGN;
    if (!grad_x && !grad_y) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int n_pad = dicp_padded_targets(n), m_pad = dicp_padded_targets(m);
    if (grad_y) {
        if ((rc = dicp_fill::zero(workspace, (size_t)N * m_pad * 3 * ts, st))) return rc;
        if ((rc = dicp_fill::zero(grad_y, (size_t)N * m * cy * ts, st))) return rc;
    }
    const int bpc = (n + BLOCK - 1) / BLOCK;
    const unsigned g = grid_for(N, bpc);
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        knn_points_bwd_kernel<T><<<g, BLOCK, 0, st>>>((const T*)g_d2, (const typename V4<T>::type*)x_tgs4, x_perm, x_rows, n, n_pad,
            (const typename V4<T>::type*)y_tgs4, m_pad, N, k, bpc, (const int32_t*)fwd_workspace, (T*)grad_x, cx, (T*)(grad_y ? workspace : nullptr));
    });
    if ((rc = launch_status()) || !grad_y) return rc;
    return dicp_permute_add_rows(dtype, workspace, y_perm, N, m_pad, m_pad, m_pad, 3, 3, grad_y, m, cy, stream);
}
