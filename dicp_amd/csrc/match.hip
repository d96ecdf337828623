// The exact k nearest rows in descriptor space and the gradient of their squared distances (dicp_knn_features, dicp_knn_features_backward,
// dicp_knn_features_backward_det; dicp_amd/match.py).  The rules per element are csrc/dicp_match.h's; nothing here forms the (n, m) matrix.
//
// Forward, two forms of one definition (score = the fma chain from h_j over the channels in ascending order):
//   match_mfma_kernel (float32)  v_mfma_f32_32x32x2_f32: A = a tile of 32 rows of y, B = -x of 32 queries, the accumulator starts at h_j of
//       its row, one MFMA per channel pair (k = 0: the even channel, k = 1: the odd one -- the instruction's own k order is the chain's; an
//       odd D is padded with the pair (y = +0, -x = -0), whose product -0 leaves s unchanged bit for bit).  The result's column is on the
//       lane and its 16 registers are 16 rows of the tile (row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)), as in knn_f16.hip's filter: a lane's
//       16 scores belong to ONE query, the running list is lane-local, and the lists of a query's two lanes (l, l ^ 32: the two halves of
//       every tile) are merged at the end.  A wave owns 32 queries (-x in NP registers per lane), a workgroup 128; y is staged through LDS in
//       stages of up to 8 tiles, channel-major with a row stride of 33 words (the transposing store and the operand load are both
//       conflict-free).  What bounds it: the MFMA issue rate (64 cycles per pair of channels per 32 x 32 scores: the f32 matrix peak, equal
//       to the f32 vector peak) plus the 16 list comparisons per lane and tile on the vector unit.
//   match_valu_kernel (float32 / float64)  one fma per channel per pair: a thread per query, 16 rows of y per LDS tile (read as
//       broadcasts), the query's channels re-read in chunks of 16 from global memory.  Bound by LDS issue (one read per fma).
// Pad rows are kept out by j < rows, never by their values; a NaN or inf in a row of either side poisons only that row's / that query's
// scores (both forms compute each score from its own two rows alone).
// The winners' d2 is recomputed from the differences (match_refine) by the lane that holds the list.
//
// Backward: match_bwd_kernel gives a wave to every query, lanes over channels: gx is the sum of the query's terms in slot order (stored
// once), gy gets -t by float atomics.  match_det_kernel gives a wave to every row of y, lanes over channels, and walks the row's list in
// the inverted index in dicp_inverse.h's order of summation (stored once, no zero fill, no atomics).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_group.h"
#include "dicp_group_launch.h"
#include "dicp_match.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MV_ROWS = 16;             // rows of y per LDS tile of the vector form
constexpr int MV_CH = 16;               // channels of the query held in registers at a time
constexpr int MM_QUERIES = 32 * (BLOCK / WAVE);     // queries per workgroup of the matrix-core form
constexpr int MM_STAGE_TILES = 8;       // at most this many 32-row tiles per LDS stage
constexpr int MM_STAGE_WORDS = 256;     // tiles x padded channels per stage
constexpr int MM_ROW_STRIDE = 33;       // words between two channels of a tile in LDS

template <typename T>
__global__ __launch_bounds__(BLOCK) void match_norm_kernel(const T* __restrict__ y, int D, size_t total, T* __restrict__ h) {
    for (size_t r = (size_t)blockIdx.x * BLOCK + threadIdx.x; r < total; r += (size_t)gridDim.x * BLOCK) h[r] = match_half_norm<T>(y + r * D, D);
}

// the list (entries K - k .. K - 1) of query row xr -> its k slots of d2 / idx
template <typename T, int K>
__device__ __forceinline__ void match_write(const T* xr, const T* yb, int D, int k, const int (&id)[K], T* __restrict__ d2o, int64_t* __restrict__ io) {
#pragma unroll
    for (int e = 0; e < K; ++e) {
        if (e >= K - k) {
            T d;
            int64_t j;
            match_output<T>(xr, yb, D, id[e], d, j);
            d2o[e - (K - k)] = d;
            io[e - (K - k)] = j;
        }
    }
}

template <typename T, int K>
__global__ __launch_bounds__(BLOCK) void match_valu_kernel(const T* __restrict__ x, const int32_t* __restrict__ x_rows, int n, const T* __restrict__ y,
                                                           const T* __restrict__ h, const int32_t* __restrict__ y_rows, int m, int D, int k, int bpc,
                                                           T* __restrict__ d2, int64_t* __restrict__ idx) {
    __shared__ T ys[MV_ROWS * MATCH_D_MAX];
    __shared__ T hs[MV_ROWS];
    const int cloud = blockIdx.x / bpc, blk = blockIdx.x % bpc;
    const int i = blk * BLOCK + (int)threadIdx.x;
    const int rows = rows_of(y_rows, cloud, m);
    const bool live = i < n, active = live && i < rows_of(x_rows, cloud, n);
    const T* xr = x + ((size_t)cloud * n + (live ? i : 0)) * D;
    const T* yb = y + (size_t)cloud * m * D;
    const T* hb = h + (size_t)cloud * m;
    T sc[K];
    int id[K], sl[K];
    topk_init<T, K>(sc, id, sl, k);
    const auto same = [](int j) { return j; };
    const auto ins = topk_inserter<T, K>(sc, id, sl, same);
    for (int base = 0; base < rows; base += MV_ROWS) {
        const int nr = min(MV_ROWS, rows - base);
        __syncthreads();
        for (int e = threadIdx.x; e < nr * D; e += BLOCK) ys[e] = yb[(size_t)base * D + e];
        if ((int)threadIdx.x < nr) hs[threadIdx.x] = hb[base + threadIdx.x];
        __syncthreads();
        T acc[MV_ROWS];
#pragma unroll
        for (int r = 0; r < MV_ROWS; ++r) acc[r] = r < nr ? hs[r] : T(0);
        for (int c0 = 0; c0 < D; c0 += MV_CH) {
            T xv[MV_CH];
#pragma unroll
            for (int u = 0; u < MV_CH; ++u) xv[u] = c0 + u < D ? xr[c0 + u] : T(0);
            if (c0 + MV_CH <= D && nr == MV_ROWS) {
#pragma unroll
                for (int u = 0; u < MV_CH; ++u) {
#pragma unroll
                    for (int r = 0; r < MV_ROWS; ++r) acc[r] = match_score_step<T>(acc[r], xv[u], ys[r * D + c0 + u]);
                }
            } else {
#pragma unroll
                for (int u = 0; u < MV_CH; ++u) {
                    if (c0 + u < D) {
#pragma unroll
                        for (int r = 0; r < MV_ROWS; ++r)
                            if (r < nr) acc[r] = match_score_step<T>(acc[r], xv[u], ys[r * D + c0 + u]);
                    }
                }
            }
        }
        if (active) {
#pragma unroll
            for (int r = 0; r < MV_ROWS; ++r)
                if (r < nr && match_finite<T>(acc[r])) ins(acc[r], base + r);
        }
    }
    if (live) match_write<T, K>(xr, yb, D, k, id, d2 + ((size_t)cloud * n + i) * k, idx + ((size_t)cloud * n + i) * k);
}

// NP: the channel pairs the kernel holds of -x (D <= 2 NP)
template <int K, int NP>
__global__ __launch_bounds__(BLOCK) void match_mfma_kernel(const float* __restrict__ x, const int32_t* __restrict__ x_rows, int n, const float* __restrict__ y,
                                                           const float* __restrict__ h, const int32_t* __restrict__ y_rows, int m, int D, int k, int bpc,
                                                           float* __restrict__ d2, int64_t* __restrict__ idx) {
    __shared__ float ys[MM_STAGE_WORDS * MM_ROW_STRIDE];
    __shared__ float hs[MM_STAGE_TILES * 32];
    const int cloud = blockIdx.x / bpc, blk = blockIdx.x % bpc;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6, col = lane & 31, kh = lane >> 5;
    const int i = (blk * (BLOCK / WAVE) + wave) * 32 + col;
    const int np = (D + 1) >> 1, Dp = 2 * np;
    const int ts = max(1, min(MM_STAGE_TILES, MM_STAGE_WORDS / Dp)), stage_rows = ts * 32;
    const int rows = rows_of(y_rows, cloud, m);
    const bool live = i < n, active = live && i < rows_of(x_rows, cloud, n);
    const float* xr = x + ((size_t)cloud * n + (live ? i : 0)) * D;
    const float* yb = y + (size_t)cloud * m * D;
    const float* hb = h + (size_t)cloud * m;
    float b[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int c = 2 * p + kh;
        b[p] = c < D ? -xr[c] : -0.0f;
    }
    float sc[K];
    int id[K], sl[K];
    topk_init<float, K>(sc, id, sl, k);
    const auto same = [](int j) { return j; };
    const auto ins = topk_inserter<float, K>(sc, id, sl, same);
    for (int base = 0; base < rows; base += stage_rows) {
        __syncthreads();
        for (int e = threadIdx.x; e < stage_rows * Dp; e += BLOCK) {
            const int rr = e / Dp, c = e - rr * Dp, j = base + rr;
            ys[((rr >> 5) * Dp + c) * MM_ROW_STRIDE + (rr & 31)] = (j < rows && c < D) ? yb[(size_t)j * D + c] : 0.0f;
        }
        if ((int)threadIdx.x < stage_rows) hs[threadIdx.x] = base + (int)threadIdx.x < rows ? hb[base + threadIdx.x] : 0.0f;
        __syncthreads();
        const int nt = min(ts, (rows - base + 31) >> 5);
        for (int t = 0; t < nt; ++t) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = hs[t * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh];
            const float* at = ys + (t * Dp + kh) * MM_ROW_STRIDE + col;
#pragma unroll
            for (int p = 0; p < NP; ++p)
                if (p < np) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(at[p * 2 * MM_ROW_STRIDE], b[p], acc, 0, 0, 0);
            if (active) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = base + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    const float s = acc[r];
                    if (j < rows && match_finite<float>(s)) ins(s, j);
                }
            }
        }
    }
    // the query's two lanes merge: lane half 0 takes the other half's entries (any order of insertion gives the same list)
#pragma unroll
    for (int e = 0; e < K; ++e) {
        const float ps = __shfl(sc[e], lane ^ 32);
        const int pj = __shfl(id[e], lane ^ 32);
        if (kh == 0 && pj >= 0) ins(ps, pj);
    }
    if (kh == 0 && live) match_write<float, K>(xr, yb, D, k, id, d2 + ((size_t)cloud * n + i) * k, idx + ((size_t)cloud * n + i) * k);
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void match_bwd_kernel(const T* __restrict__ g, const int64_t* __restrict__ idx, const T* __restrict__ x,
                                                          const T* __restrict__ y, int n, int m, int D, int k, size_t queries,
                                                          T* __restrict__ gx, T* __restrict__ gy) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    for (size_t q = (size_t)blockIdx.x * (BLOCK / WAVE) + wave; q < queries; q += (size_t)gridDim.x * (BLOCK / WAVE)) {
        const size_t b = q / n;
        const T* gq = g + q * k;
        const int64_t* iq = idx + q * k;
        const T* yb = y + b * m * D;
        for (int c = lane; c < D; c += WAVE) {
            const T xc = x[q * D + c];
            if (!gy) {
                gx[q * D + c] = match_grad_x<T>(gq, iq, k, xc, yb, D, m, c);
                continue;
            }
            T sum = T(0);
            for (int s = 0; s < k; ++s) {
                const int j = group_row(iq[s], m);
                if (j < 0 || gq[s] == T(0)) continue;
                const T t = match_term<T>(gq[s], xc, yb[(size_t)j * D + c]);
                sum = sum + t;
                unsafeAtomicAdd(gy + (b * m + j) * D + c, -t);
            }
            if (gx) gx[q * D + c] = sum;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void match_det_kernel(const T* __restrict__ g, const int64_t* __restrict__ idx, const int32_t* __restrict__ y_rows,
                                                          const T* __restrict__ x, const T* __restrict__ y, int n, int m, int D, int k,
                                                          const int32_t* __restrict__ offsets, const int32_t* __restrict__ slots, size_t total,
                                                          T* __restrict__ gy) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const size_t nk = (size_t)n * k;
    for (size_t r = (size_t)blockIdx.x * (BLOCK / WAVE) + wave; r < total; r += (size_t)gridDim.x * (BLOCK / WAVE)) {
        const size_t b = r / m;
        const int j = (int)(r - b * m);
        const int rows = rows_of(y_rows, (int)b, m);
        int lo = 0, hi = 0;
        if (j < rows) det_list(offsets + b * ((size_t)m + 1), j, (int)nk, lo, hi);
        for (int c = lane; c < D; c += WAVE)
            gy[r * D + c] = match_det_sum<T>(g + b * nk, idx + b * nk, x + b * n * D, n, k, D, rows, slots + b * nk, j, y[r * D + c], c, lo, hi);
    }
}

// the checks the three entry points share, after the null checks: dtype, then the shape
inline int match_check(int dtype, int N, int n, int m, int D, int k) {
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (N < 1 || n < 1 || m < 1 || D < 1 || D > MATCH_D_MAX || k < 1 || k > MATCH_K_MAX) return DICP_ERR_SHAPE;
    if (n > (1 << 30) || m > (1 << 30) || (size_t)n * k >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;     // row and slot numbers are int32
    if ((size_t)N * ((size_t)(n + MM_QUERIES - 1) / MM_QUERIES) >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;   // the grid
    if (!fits62((size_t)N * n, 8, (size_t)D) || !fits62((size_t)N * m, 8, (size_t)D) || !fits62((size_t)N * n, 8, (size_t)k)) return DICP_ERR_SHAPE;
    return 0;
}

template <int K>
void launch_mfma(int np, unsigned grid, hipStream_t st, const float* x, const int32_t* x_rows, int n, const float* y, const float* h,
                 const int32_t* y_rows, int m, int D, int k, int bpc, float* d2, int64_t* idx) {
    if (np <= 16) match_mfma_kernel<K, 16><<<grid, BLOCK, 0, st>>>(x, x_rows, n, y, h, y_rows, m, D, k, bpc, d2, idx);
    else if (np <= 32) match_mfma_kernel<K, 32><<<grid, BLOCK, 0, st>>>(x, x_rows, n, y, h, y_rows, m, D, k, bpc, d2, idx);
    else if (np <= 64) match_mfma_kernel<K, 64><<<grid, BLOCK, 0, st>>>(x, x_rows, n, y, h, y_rows, m, D, k, bpc, d2, idx);
    else match_mfma_kernel<K, 128><<<grid, BLOCK, 0, st>>>(x, x_rows, n, y, h, y_rows, m, D, k, bpc, d2, idx);
}

}  // namespace

size_t dicp_knn_features_workspace_bytes(int dtype, int N, int m) {
    if (bad_dtype(dtype) || N < 1 || m < 1) return 0;
    return up256((size_t)N * m * elem_size(dtype));
}

int dicp_knn_features(int dtype, const void* x, const int32_t* x_rows, int n, const void* y, const int32_t* y_rows, int m, int D, int N, int k,
                      int form, void* d2, int64_t* idx, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !y || !d2 || !idx || !workspace) return DICP_ERR_NULL;
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (form != MATCH_FORM_AUTO && form != MATCH_FORM_VALU && form != MATCH_FORM_MFMA) return DICP_ERR_ENUM;
    if (form == MATCH_FORM_MFMA && dtype != DICP_F32) return DICP_ERR_ENUM;
    if (const int bad = match_check(dtype, N, n, m, D, k)) return bad;
    if (workspace_bytes < dicp_knn_features_workspace_bytes(dtype, N, m)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(x, ts) || misaligned(y, ts) || misaligned(d2, ts) || misaligned(idx, 8) || misaligned(x_rows, 4) || misaligned(y_rows, 4) ||
        misaligned(workspace, 16)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const bool mfma = dtype == DICP_F32 && form != MATCH_FORM_VALU;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        match_norm_kernel<T><<<grid_1d((size_t)N * m), BLOCK, 0, st>>>((const T*)y, D, (size_t)N * m, (T*)workspace);
    });
    if (mfma) {
        const int bpc = (n + MM_QUERIES - 1) / MM_QUERIES;
        topk_with_kcap(k, [&](auto kc) {
            launch_mfma<decltype(kc)::value>((D + 1) / 2, (unsigned)N * (unsigned)bpc, st, (const float*)x, x_rows, n, (const float*)y, (const float*)workspace,
                                             y_rows, m, D, k, bpc, (float*)d2, idx);
        });
    } else {
        const int bpc = (n + BLOCK - 1) / BLOCK;
        with_scalar(dtype, [&](auto t) {
            using T = decltype(t);
            topk_with_kcap(k, [&](auto kc) {
                match_valu_kernel<T, decltype(kc)::value><<<(unsigned)N * (unsigned)bpc, BLOCK, 0, st>>>((const T*)x, x_rows, n, (const T*)y, (const T*)workspace,
                                                                                                       y_rows, m, D, k, bpc, (T*)d2, idx);
            });
        });
    }
    return launch_status();
}

int dicp_knn_features_backward(int dtype, const void* g_d2, const int64_t* idx, const void* x, const void* y, int n, int m, int D, int N, int k,
                               void* grad_x, void* grad_y, void* stream) {
    if (!g_d2 || !idx || !x || !y) return DICP_ERR_NULL;
    if (const int bad = match_check(dtype, N, n, m, D, k)) return bad;
    const size_t ts = elem_size(dtype);
    if (misaligned(g_d2, ts) || misaligned(x, ts) || misaligned(y, ts) || misaligned(grad_x, ts) || misaligned(grad_y, ts) || misaligned(idx, 8))
        return DICP_ERR_ALIGN;
    if (!grad_x && !grad_y) return 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t queries = (size_t)N * n;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        match_bwd_kernel<T><<<group_grid(queries, BLOCK / WAVE), BLOCK, 0, st>>>((const T*)g_d2, idx, (const T*)x, (const T*)y, n, m, D, k, queries,
                                                                                (T*)grad_x, (T*)grad_y);
    });
    return launch_status();
}

int dicp_knn_features_backward_det(int dtype, const void* g_d2, const int64_t* idx, const int32_t* y_rows, const void* x, const void* y, int n, int m,
                                   int D, int N, int k, const int32_t* offsets, const int32_t* slots, void* grad_y, void* stream) {
    if (!g_d2 || !idx || !x || !y || !offsets || !slots || !grad_y) return DICP_ERR_NULL;
    if (const int bad = match_check(dtype, N, n, m, D, k)) return bad;
    const size_t ts = elem_size(dtype);
    if (misaligned(g_d2, ts) || misaligned(x, ts) || misaligned(y, ts) || misaligned(grad_y, ts) || misaligned(idx, 8) || misaligned(y_rows, 4) ||
        misaligned(offsets, 4) || misaligned(slots, 4)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const size_t total = (size_t)N * m;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        match_det_kernel<T><<<group_grid(total, BLOCK / WAVE), BLOCK, 0, st>>>((const T*)g_d2, idx, y_rows, (const T*)x, (const T*)y, n, m, D, k, offsets,
                                                                              slots, total, (T*)grad_y);
    });
    return launch_status();
}
