// Soft descriptor matches: out_i = sum_j softmax_j(-|fx_i - fy_j|^2 / tau) values_j, with the hard winner and its probability, and the
// gradients of out in both descriptor tables and the values (dicp_soft_match, dicp_soft_match_backward; dicp_amd/match.py:
// soft_match_features).  The rules per element are csrc/dicp_softmatch.h's on the score of csrc/dicp_match.h; nothing here forms or stores
// the (n, m) matrix.
//
// Forward, two forms of one definition:
//   soft_mfma_kernel (float32)  the scores as match.hip's match_mfma_kernel makes them: v_mfma_f32_32x32x2_f32, A = a tile of 32 rows of
//       fy, B = -fx of 32 queries, the accumulator started at h_j, one MFMA per channel pair; fy staged channel-major through LDS (row
//       stride 33 words) in stages of up to 8 tiles, h and the value rows (padded to CC columns) beside it.  A lane's 16 scores belong to
//       ONE query (row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the tile): they are one block of the lane's online softmax -- the block's
//       maximum raises the running maximum once, then one exp per score -- and the running (score, index) minimum is lane-local too.
//       The two lanes of a query (l, l ^ 32) are joined at the end (soft_merge).
//   soft_valu_kernel (float32 / float64)  a thread per query, 16 rows of fy per LDS tile = one block, the query's channels re-read in
//       chunks of 16 from global memory; the order of csrc/dicp_softmatch.h's soft_query.
// The two forms walk the rows in different orders, so their sums differ in the last bits; the decisions (idx, the candidates) do not.
//
// Backward: the scores are recomputed by the same chain, p from the saved lse; one pass owns the queries, one the rows of fy.
//   soft_bwd_mfma_kernel (float32, D <= 128)  both passes on the matrix cores: see the kernel.
//   soft_bwd_q_kernel / soft_bwd_t_kernel (float32 / float64)  the vector unit: a thread per query (per row of fy) and chunk of SB_CH
//       channels, the other table through LDS (the queries with their cotangent, lse and delta).  A call with D > SB_CH recomputes the
//       scores once per chunk.
// No atomics, every element stored once, no zero fill.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_group_launch.h"
#include "dicp_softmatch.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SV_CH = 16;               // channels of the thread's own row held in registers at a time (vector forms)
constexpr int SB_CH = 64;               // channels of a gradient row a thread of the backward accumulates
constexpr int SM_QUERIES = 32 * (BLOCK / WAVE);     // queries per workgroup of the matrix-core form
constexpr int SM_STAGE_TILES = 8;       // at most this many 32-row tiles per LDS stage
constexpr int SM_STAGE_WORDS = 256;     // tiles x padded channels per stage
constexpr int SM_ROW_STRIDE = 33;       // words between two channels of a tile in LDS
constexpr int SOFT_BWD_MFMA_D = 128;    // the matrix-core backward keeps D / 32 accumulator tiles per lane: up to this D

template <typename T>
__global__ __launch_bounds__(BLOCK) void soft_norm_kernel(const T* __restrict__ y, int D, size_t total, T* __restrict__ h) {
    for (size_t r = (size_t)blockIdx.x * BLOCK + threadIdx.x; r < total; r += (size_t)gridDim.x * BLOCK) h[r] = match_half_norm<T>(y + r * D, D);
}

template <typename T, int CC>
__device__ __forceinline__ void soft_write(const SoftState<T, CC>& q, T c, int C, size_t row, T* __restrict__ out, T* __restrict__ lse,
                                           int64_t* __restrict__ idx, T* __restrict__ prob) {
    T o[CC];
    soft_finish<T, CC>(q, c, o, lse[row], idx[row], prob[row]);
#pragma unroll
    for (int k = 0; k < CC; ++k)
        if (k < C) out[row * C + k] = o[k];
}

// the scores of the thread's row against the 16 rows of an LDS tile ts (row-major, D channels): acc[r] starts at start(r)
template <typename T, typename Start>
__device__ __forceinline__ void tile_scores(const T* own, bool own_is_x, const T* ts, int nr, int D, const Start& start, T (&acc)[SOFT_ROWS]) {
#pragma unroll
    for (int r = 0; r < SOFT_ROWS; ++r) acc[r] = r < nr ? start(r) : T(0);
    for (int c0 = 0; c0 < D; c0 += SV_CH) {
        T ov[SV_CH];
#pragma unroll
        for (int u = 0; u < SV_CH; ++u) ov[u] = c0 + u < D ? own[c0 + u] : T(0);
#pragma unroll
        for (int u = 0; u < SV_CH; ++u) {
            if (c0 + u < D) {
#pragma unroll
                for (int r = 0; r < SOFT_ROWS; ++r) {
                    if (r < nr) {
                        const T t = ts[r * D + c0 + u];
                        acc[r] = own_is_x ? match_score_step<T>(acc[r], ov[u], t) : match_score_step<T>(acc[r], t, ov[u]);
                    }
                }
            }
        }
    }
}

// G[u] = fma(a, row[u], G[u]) for the nu <= SB_CH channels of a chunk (nu is uniform over the workgroup), in halves of 32
template <typename T>
__device__ __forceinline__ void row_fma(T (&G)[SB_CH], T a, const T* row, int nu) {
#pragma unroll
    for (int h = 0; h < SB_CH; h += 32) {
        if (nu >= h + 32) {
#pragma unroll
            for (int u = 0; u < 32; ++u) G[h + u] = match_fma(a, row[h + u], G[h + u]);
        } else if (nu > h) {
#pragma unroll
            for (int u = 0; u < 32; ++u)
                if (h + u < nu) G[h + u] = match_fma(a, row[h + u], G[h + u]);
        }
    }
}

template <typename T, int CC>
__global__ __launch_bounds__(BLOCK) void soft_valu_kernel(const T* __restrict__ x, const int32_t* __restrict__ x_rows, int n, const T* __restrict__ y,
                                                          const T* __restrict__ h, const T* __restrict__ values, const int32_t* __restrict__ y_rows, int m,
                                                          int D, int C, int bpc, T c, T* __restrict__ out, T* __restrict__ lse, int64_t* __restrict__ idx,
                                                          T* __restrict__ prob) {
    __shared__ T ys[SOFT_ROWS * MATCH_D_MAX];
    __shared__ T hs[SOFT_ROWS];
    __shared__ T vs[SOFT_ROWS * CC];
    const int cloud = blockIdx.x / bpc, blk = blockIdx.x % bpc;
    const int i = blk * BLOCK + (int)threadIdx.x;
    const int rows = rows_of(y_rows, cloud, m);
    const bool live = i < n, active = live && i < rows_of(x_rows, cloud, n);
    const T* xr = x + ((size_t)cloud * n + (live ? i : 0)) * D;
    const T* yb = y + (size_t)cloud * m * D;
    const T* hb = h + (size_t)cloud * m;
    const T* vb = values + (size_t)cloud * m * C;
    SoftState<T, CC> q;
    soft_init<T, CC>(q);
    for (int base = 0; base < rows; base += SOFT_ROWS) {
        const int nr = min(SOFT_ROWS, rows - base);
        __syncthreads();
        for (int e = threadIdx.x; e < nr * D; e += BLOCK) ys[e] = yb[(size_t)base * D + e];
        if ((int)threadIdx.x < nr) hs[threadIdx.x] = hb[base + threadIdx.x];
        if ((int)threadIdx.x < nr * CC) {
            const int r = threadIdx.x / CC, k = threadIdx.x % CC;
            vs[threadIdx.x] = k < C ? vb[(size_t)(base + r) * C + k] : T(0);
        }
        __syncthreads();
        T acc[SOFT_ROWS];
        tile_scores<T>(xr, true, ys, nr, D, [&](int r) { return hs[r]; }, acc);
        if (active) {
            T l[SOFT_ROWS], Mb = -soft_inf<T>();
#pragma unroll
            for (int r = 0; r < SOFT_ROWS; ++r) {
                l[r] = soft_logit<T>(c, acc[r]);
                if (r < nr && match_finite<T>(acc[r]) && l[r] > Mb) Mb = l[r];
            }
            soft_raise<T, CC>(q, Mb);
#pragma unroll
            for (int r = 0; r < SOFT_ROWS; ++r)
                if (r < nr && match_finite<T>(acc[r])) soft_add<T, CC>(q, acc[r], l[r], base + r, vs + r * CC);
        }
    }
    if (live) soft_write<T, CC>(q, c, C, (size_t)cloud * n + i, out, lse, idx, prob);
}

// NP: the channel pairs the kernel holds of -x (D <= 2 NP)
template <int NP, int CC>
__global__ __launch_bounds__(BLOCK) void soft_mfma_kernel(const float* __restrict__ x, const int32_t* __restrict__ x_rows, int n, const float* __restrict__ y,
                                                          const float* __restrict__ h, const float* __restrict__ values, const int32_t* __restrict__ y_rows,
                                                          int m, int D, int C, int bpc, float c, float* __restrict__ out, float* __restrict__ lse,
                                                          int64_t* __restrict__ idx, float* __restrict__ prob) {
    __shared__ float ys[SM_STAGE_WORDS * SM_ROW_STRIDE];
    __shared__ float hs[SM_STAGE_TILES * 32];
    __shared__ float vs[SM_STAGE_TILES * 32 * CC];
    const int cloud = blockIdx.x / bpc, blk = blockIdx.x % bpc;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6, col = lane & 31, kh = lane >> 5;
    const int i = (blk * (BLOCK / WAVE) + wave) * 32 + col;
    const int np = (D + 1) >> 1, Dp = 2 * np;
    const int ts = max(1, min(SM_STAGE_TILES, SM_STAGE_WORDS / Dp)), stage_rows = ts * 32;
    const int rows = rows_of(y_rows, cloud, m);
    const bool live = i < n, active = live && i < rows_of(x_rows, cloud, n);
    const float* xr = x + ((size_t)cloud * n + (live ? i : 0)) * D;
    const float* yb = y + (size_t)cloud * m * D;
    const float* hb = h + (size_t)cloud * m;
    const float* vb = values + (size_t)cloud * m * C;
    float b[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int ch = 2 * p + kh;
        b[p] = ch < D ? -xr[ch] : -0.0f;
    }
    SoftState<float, CC> q;
    soft_init<float, CC>(q);
    for (int base = 0; base < rows; base += stage_rows) {
        __syncthreads();
        for (int e = threadIdx.x; e < stage_rows * Dp; e += BLOCK) {
            const int rr = e / Dp, ch = e - rr * Dp, j = base + rr;
            ys[((rr >> 5) * Dp + ch) * SM_ROW_STRIDE + (rr & 31)] = (j < rows && ch < D) ? yb[(size_t)j * D + ch] : 0.0f;
        }
        if ((int)threadIdx.x < stage_rows) hs[threadIdx.x] = base + (int)threadIdx.x < rows ? hb[base + threadIdx.x] : 0.0f;
        for (int e = threadIdx.x; e < stage_rows * CC; e += BLOCK) {
            const int rr = e / CC, k = e - rr * CC, j = base + rr;
            vs[e] = (j < rows && k < C) ? vb[(size_t)j * C + k] : 0.0f;
        }
        __syncthreads();
        const int nt = min(ts, (rows - base + 31) >> 5);
        for (int t = 0; t < nt; ++t) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = hs[t * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh];
            const float* at = ys + (t * Dp + kh) * SM_ROW_STRIDE + col;
#pragma unroll
            for (int p = 0; p < NP; ++p)
                if (p < np) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(at[p * 2 * SM_ROW_STRIDE], b[p], acc, 0, 0, 0);
            if (active) {
                float l[16], Mb = -soft_inf<float>();
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = base + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    l[r] = soft_logit<float>(c, acc[r]);
                    if (j < rows && match_finite<float>(acc[r]) && l[r] > Mb) Mb = l[r];
                }
                soft_raise<float, CC>(q, Mb);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int tr = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    if (base + tr < rows && match_finite<float>(acc[r])) soft_add<float, CC>(q, acc[r], l[r], base + tr, vs + tr * CC);
                }
            }
        }
    }
    // the query's two lanes: lane half 0 takes the other half's state
    SoftState<float, CC> o;
    o.M = __shfl(q.M, lane ^ 32);
    o.S = __shfl(q.S, lane ^ 32);
#pragma unroll
    for (int k = 0; k < CC; ++k) o.a[k] = __shfl(q.a[k], lane ^ 32);
    o.bs = __shfl(q.bs, lane ^ 32);
    o.bj = __shfl(q.bj, lane ^ 32);
    if (kh == 0 && live) {
        soft_merge<float, CC>(q, o);
        soft_write<float, CC>(q, c, C, (size_t)cloud * n + i, out, lse, idx, prob);
    }
}

// grid: (cloud, block of BLOCK queries, chunk of SB_CH channels), the chunk fastest
template <typename T, int CC>
__global__ __launch_bounds__(BLOCK) void soft_bwd_q_kernel(const T* __restrict__ x, const int32_t* __restrict__ x_rows, int n, const T* __restrict__ y,
                                                           const T* __restrict__ h, const T* __restrict__ values, const int32_t* __restrict__ y_rows, int m,
                                                           int D, int C, int bpc, int nch, T c, const T* __restrict__ out, const T* __restrict__ lse,
                                                           const T* __restrict__ g, T* __restrict__ gx) {
    __shared__ T ys[SOFT_ROWS * MATCH_D_MAX];
    __shared__ T hs[SOFT_ROWS];
    __shared__ T vs[SOFT_ROWS * CC];
    const int ch0 = (int)(blockIdx.x % nch) * SB_CH, rest = blockIdx.x / nch;
    const int cloud = rest / bpc, blk = rest % bpc;
    const int i = blk * BLOCK + (int)threadIdx.x;
    const int rows = rows_of(y_rows, cloud, m);
    const bool live = i < n;
    const size_t qr = (size_t)cloud * n + (live ? i : 0);
    const T L = lse[qr];
    const bool active = live && i < rows_of(x_rows, cloud, n) && soft_live<T>(L);
    const T* xr = x + qr * D;
    const T* yb = y + (size_t)cloud * m * D;
    const T* hb = h + (size_t)cloud * m;
    const T* vb = values + (size_t)cloud * m * C;
    T go[CC], o[CC];
#pragma unroll
    for (int k = 0; k < CC; ++k) {
        go[k] = k < C ? g[qr * C + k] : T(0);
        o[k] = k < C ? out[qr * C + k] : T(0);
    }
    const T delta = soft_dot<T, CC>(go, o);
    const int nu = min(SB_CH, D - ch0);
    T G[SB_CH];
#pragma unroll
    for (int u = 0; u < SB_CH; ++u) G[u] = T(0);
    for (int base = 0; base < rows; base += SOFT_ROWS) {
        const int nr = min(SOFT_ROWS, rows - base);
        __syncthreads();
        for (int e = threadIdx.x; e < nr * D; e += BLOCK) ys[e] = yb[(size_t)base * D + e];
        if ((int)threadIdx.x < nr) hs[threadIdx.x] = hb[base + threadIdx.x];
        if ((int)threadIdx.x < nr * CC) {
            const int r = threadIdx.x / CC, k = threadIdx.x % CC;
            vs[threadIdx.x] = k < C ? vb[(size_t)(base + r) * C + k] : T(0);
        }
        __syncthreads();
        T acc[SOFT_ROWS];
        tile_scores<T>(xr, true, ys, nr, D, [&](int r) { return hs[r]; }, acc);
        if (!active) continue;
        for (int r = 0; r < nr; ++r) {
            T s = acc[0];
#pragma unroll
            for (int e = 1; e < SOFT_ROWS; ++e) s = e == r ? acc[e] : s;
            if (!match_finite<T>(s)) continue;
            const T a = soft_a<T>(soft_prob<T>(c, s, L), soft_dot<T, CC>(go, vs + r * CC), delta);
            row_fma<T>(G, a, ys + r * D + ch0, nu);
        }
    }
    if (live) {
#pragma unroll
        for (int u = 0; u < SB_CH; ++u)
            if (u < nu) gx[qr * D + ch0 + u] = active ? soft_grad_x<T>(c, G[u]) : T(0);
    }
}

// grid: (cloud, block of BLOCK rows of fy, chunk of SB_CH channels), the chunk fastest; chunk 0 also owns the row's gvalues
template <typename T, int CC>
__global__ __launch_bounds__(BLOCK) void soft_bwd_t_kernel(const T* __restrict__ x, const int32_t* __restrict__ x_rows, int n, const T* __restrict__ y,
                                                           const T* __restrict__ h, const T* __restrict__ values, const int32_t* __restrict__ y_rows, int m,
                                                           int D, int C, int bpc, int nch, T c, const T* __restrict__ out, const T* __restrict__ lse,
                                                           const T* __restrict__ g, T* __restrict__ gy, T* __restrict__ gv) {
    __shared__ T xs[SOFT_ROWS * MATCH_D_MAX];
    __shared__ T gs[SOFT_ROWS * CC];
    __shared__ T Ls[SOFT_ROWS];
    __shared__ T ds[SOFT_ROWS];
    const int chunk = (int)(blockIdx.x % nch), ch0 = chunk * SB_CH, rest = blockIdx.x / nch;
    const int cloud = rest / bpc, blk = rest % bpc;
    const int j = blk * BLOCK + (int)threadIdx.x;
    const int qrows = rows_of(x_rows, cloud, n);
    const bool live = j < m, on = live && j < rows_of(y_rows, cloud, m);
    const size_t tr = (size_t)cloud * m + (live ? j : 0);
    const T* yr = y + tr * D;
    const T* xb = x + (size_t)cloud * n * D;
    const T hj = h[tr];
    T vj[CC], GV[CC];
#pragma unroll
    for (int k = 0; k < CC; ++k) {
        vj[k] = (on && k < C) ? values[tr * C + k] : T(0);
        GV[k] = T(0);
    }
    const int nu = min(SB_CH, D - ch0);
    T A[SB_CH], sa = T(0);
    bool any = false;                   // a row nobody weighs (a non-finite one among them) gets exactly zero
#pragma unroll
    for (int u = 0; u < SB_CH; ++u) A[u] = T(0);
    for (int base = 0; base < qrows; base += SOFT_ROWS) {
        const int nr = min(SOFT_ROWS, qrows - base);
        __syncthreads();
        for (int e = threadIdx.x; e < nr * D; e += BLOCK) xs[e] = xb[(size_t)base * D + e];
        if ((int)threadIdx.x < nr) {
            const size_t qr = (size_t)cloud * n + base + threadIdx.x;
            T go[CC], o[CC];
#pragma unroll
            for (int k = 0; k < CC; ++k) {
                go[k] = k < C ? g[qr * C + k] : T(0);
                o[k] = k < C ? out[qr * C + k] : T(0);
                gs[threadIdx.x * CC + k] = go[k];
            }
            Ls[threadIdx.x] = lse[qr];
            ds[threadIdx.x] = soft_dot<T, CC>(go, o);
        }
        __syncthreads();
        T acc[SOFT_ROWS];
        tile_scores<T>(yr, false, xs, nr, D, [&](int) { return hj; }, acc);
        if (!on) continue;
        for (int r = 0; r < nr; ++r) {
            T s = acc[0];
#pragma unroll
            for (int e = 1; e < SOFT_ROWS; ++e) s = e == r ? acc[e] : s;
            const T L = Ls[r];
            if (!soft_live<T>(L) || !match_finite<T>(s)) continue;
            const T p = soft_prob<T>(c, s, L);
            const T a = soft_a<T>(p, soft_dot<T, CC>(gs + r * CC, vj), ds[r]);
            any = true;
            sa = sa + a;
#pragma unroll
            for (int k = 0; k < CC; ++k) GV[k] = match_fma(p, gs[r * CC + k], GV[k]);
            row_fma<T>(A, a, xs + r * D + ch0, nu);
        }
    }
    if (live) {
        if (gy) {
#pragma unroll
            for (int u = 0; u < SB_CH; ++u)
                if (u < nu) gy[tr * D + ch0 + u] = any ? soft_grad_y<T>(c, yr[ch0 + u], sa, A[u]) : T(0);
        }
        if (gv && chunk == 0) {
#pragma unroll
            for (int k = 0; k < CC; ++k)
                if (k < C) gv[tr * C + k] = any ? GV[k] : T(0);
        }
    }
}

// The backward with every product on the matrix cores (float32, D <= 2 NP <= 128).  One kernel serves both passes: the OWNER table is on
// the lanes (OWN_Y = false: the queries, B = -fx; true: the rows of fy, B = fy), the other table STREAMS through LDS channel-major as in
// soft_mfma_kernel (fy, or -fx), with the per-row extras beside it (values and h of a row of fy; the cotangent, lse and delta of a query).
// The score tile is the forward's (the same products in the same order: the same bits); a lane's 16 weights a_ij are then the B operand
// of the gradient products as they stand -- register r of lane half kh is streamed row (r & 3) + 8 (r >> 2) + 4 kh, the MFMA's k = kh -- with
// A = the streamed table's channels read back from the same LDS image: G[ch][owner] += streamed[row][ch] a[row][owner], one MFMA per
// pair of rows and block of 32 channels, the accumulators in registers for the whole sweep.  A streamed row that takes no part (past the
// count, a row of fy with a non-finite h, a query whose lse is the mark) is staged as zeros, so that its weight 0 meets no NaN.
// The sums run over the streamed rows in the tiles' register order (rows 0 4 1 5 2 6 3 7 8 12 ...), sa and gvalues per lane half, the halves
// added at the end.
template <int NP, int CC, bool OWN_Y>
__global__ __launch_bounds__(BLOCK) void soft_bwd_mfma_kernel(const float* __restrict__ x, const int32_t* __restrict__ x_rows, int n, const float* __restrict__ y,
                                                              const float* __restrict__ h, const float* __restrict__ values, const int32_t* __restrict__ y_rows,
                                                              int m, int D, int C, int bpc, float c, const float* __restrict__ out, const float* __restrict__ lse,
                                                              const float* __restrict__ g, float* __restrict__ gown, float* __restrict__ gv) {
    constexpr int NB = NP / 16;         // blocks of 32 channels
    constexpr int AUX = CC + 2;
    __shared__ float ys[SM_STAGE_WORDS * SM_ROW_STRIDE];
    __shared__ float aux[SM_STAGE_TILES * 32 * AUX];
    const int cloud = blockIdx.x / bpc, blk = blockIdx.x % bpc;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6, col = lane & 31, kh = lane >> 5;
    const int i = (blk * (BLOCK / WAVE) + wave) * 32 + col;
    const int np = (D + 1) >> 1, Dp = 2 * np;
    const int ts = max(1, min(SM_STAGE_TILES, SM_STAGE_WORDS / Dp)), stage_rows = ts * 32;
    const int xrows = rows_of(x_rows, cloud, n), yrows = rows_of(y_rows, cloud, m);
    const int nown = OWN_Y ? m : n, own_rows = OWN_Y ? yrows : xrows, str_rows = OWN_Y ? xrows : yrows;
    const bool live = i < nown;
    const size_t orow = (size_t)cloud * nown + (live ? i : 0);
    const float* own = (OWN_Y ? y : x) + orow * D;
    const float* xb = x + (size_t)cloud * n * D;
    const float* yb = y + (size_t)cloud * m * D;
    const float* hb = h + (size_t)cloud * m;
    const float* vb = values + (size_t)cloud * m * C;
    const size_t q0 = (size_t)cloud * n;
    // the owner's constants: a query's cotangent, delta and lse; a row's values and h
    float ov[CC], o2 = 0.0f, o3 = 0.0f;
    bool active = live && i < own_rows;
    if (OWN_Y) {
#pragma unroll
        for (int k = 0; k < CC; ++k) ov[k] = (active && k < C) ? values[orow * C + k] : 0.0f;
        o3 = h[orow];
    } else {
        float o[CC];
#pragma unroll
        for (int k = 0; k < CC; ++k) {
            ov[k] = k < C ? g[orow * C + k] : 0.0f;
            o[k] = k < C ? out[orow * C + k] : 0.0f;
        }
        o2 = soft_dot<float, CC>(ov, o);
        o3 = lse[orow];
        active = active && soft_live<float>(o3);
    }
    float b[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int ch = 2 * p + kh;
        b[p] = ch < D ? (OWN_Y ? own[ch] : -own[ch]) : (OWN_Y ? 0.0f : -0.0f);
    }
    f32x16 G[NB];
#pragma unroll
    for (int cb = 0; cb < NB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) G[cb][r] = 0.0f;
    float sa = 0.0f, GV[CC];
#pragma unroll
    for (int k = 0; k < CC; ++k) GV[k] = 0.0f;
    bool any = false;
    for (int base = 0; base < str_rows; base += stage_rows) {
        __syncthreads();
        if ((int)threadIdx.x < stage_rows) {
            const int j = base + (int)threadIdx.x;
            float* ar = aux + threadIdx.x * AUX;
            const bool in = j < str_rows;
            if (OWN_Y) {
                float go[CC], o[CC];
#pragma unroll
                for (int k = 0; k < CC; ++k) {
                    go[k] = (in && k < C) ? g[(q0 + j) * C + k] : 0.0f;
                    o[k] = (in && k < C) ? out[(q0 + j) * C + k] : 0.0f;
                    ar[k] = go[k];
                }
                ar[CC] = in ? lse[q0 + j] : soft_inf<float>();
                ar[CC + 1] = soft_dot<float, CC>(go, o);
            } else {
#pragma unroll
                for (int k = 0; k < CC; ++k) ar[k] = (in && k < C) ? vb[(size_t)j * C + k] : 0.0f;
                ar[CC] = in ? hb[j] : soft_inf<float>();
                ar[CC + 1] = 0.0f;
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < stage_rows * Dp; e += BLOCK) {
            const int rr = e / Dp, ch = e - rr * Dp, j = base + rr;
            const float mark = aux[rr * AUX + CC];              // h of the row of fy / lse of the query: not finite = the row takes no part
            const bool in = j < str_rows && ch < D && match_finite<float>(mark);
            const float val = in ? (OWN_Y ? -xb[(size_t)j * D + ch] : yb[(size_t)j * D + ch]) : (OWN_Y ? -0.0f : 0.0f);
            ys[((rr >> 5) * Dp + ch) * SM_ROW_STRIDE + (rr & 31)] = val;
        }
        __syncthreads();
        const int nt = min(ts, (str_rows - base + 31) >> 5);
        for (int t = 0; t < nt; ++t) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = OWN_Y ? o3 : aux[(t * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh) * AUX + CC];
            const float* at = ys + (t * Dp + kh) * SM_ROW_STRIDE + col;
#pragma unroll
            for (int p = 0; p < NP; ++p)
                if (p < np) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(at[p * 2 * SM_ROW_STRIDE], b[p], acc, 0, 0, 0);
            float a[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int tr = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                const float* ar = aux + tr * AUX;
                const float s = acc[r];
                a[r] = 0.0f;
                if (active && base + tr < str_rows && match_finite<float>(s) && match_finite<float>(ar[CC])) {
                    if (OWN_Y) {
                        const float p = soft_prob<float>(c, s, ar[CC]);
                        a[r] = soft_a<float>(p, soft_dot<float, CC>(ar, ov), ar[CC + 1]);
                        any = true;
                        sa = sa + a[r];
#pragma unroll
                        for (int k = 0; k < CC; ++k) GV[k] = match_fma(p, ar[k], GV[k]);
                    } else {
                        a[r] = soft_a<float>(soft_prob<float>(c, s, o3), soft_dot<float, CC>(ov, ar), o2);
                    }
                }
            }
#pragma unroll
            for (int cb = 0; cb < NB; ++cb) {
                const int ch = cb * 32 + col;
                if (cb * 32 < D) {
                    const float* gt = ys + (t * Dp + (ch < Dp ? ch : 0)) * SM_ROW_STRIDE + 4 * kh;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float av = ch < D ? gt[(r & 3) + 8 * (r >> 2)] : 0.0f;
                        G[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, a[r], G[cb], 0, 0, 0);
                    }
                }
            }
        }
    }
    // the two lanes of an owner hold different channels of G; sa, gvalues and `any` are per half: half 0 + half 1
    const float sa1 = __shfl(sa, lane ^ 32);
    const int any1 = __shfl((int)any, lane ^ 32);
    float GV1[CC];
#pragma unroll
    for (int k = 0; k < CC; ++k) GV1[k] = __shfl(GV[k], lane ^ 32);
    if (!live) return;
    if (OWN_Y) {
        const float st = kh == 0 ? sa + sa1 : sa1 + sa;
        const bool some = any || any1;
        if (gown) {
#pragma unroll
            for (int cb = 0; cb < NB; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ch = cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    if (ch < D) gown[orow * D + ch] = some ? c * match_fma(own[ch], st, G[cb][r]) : 0.0f;       // (G = -sum a x: -fx was staged)
                }
        }
        if (gv && kh == 0) {
#pragma unroll
            for (int k = 0; k < CC; ++k)
                if (k < C) gv[orow * C + k] = some ? GV[k] + GV1[k] : 0.0f;
        }
    } else {
#pragma unroll
        for (int cb = 0; cb < NB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ch = cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (ch < D) gown[orow * D + ch] = active ? soft_grad_x<float>(c, G[cb][r]) : 0.0f;
            }
    }
}

// the checks the two entry points share, after the null checks: dtype, then the shape
inline int soft_check(int dtype, int N, int n, int m, int D, int C, double tau) {
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (N < 1 || n < 1 || m < 1 || D < 1 || D > MATCH_D_MAX || C < 1 || C > SOFT_C_MAX) return DICP_ERR_SHAPE;
    if (!(tau > 0.0) || !(tau < (double)__builtin_huge_val())) return DICP_ERR_SHAPE;
    const double c = dtype == DICP_F32 ? (double)soft_scale<float>(tau) : soft_scale<double>(tau);
    if (!(c < 0.0) || !(c > -(double)__builtin_huge_val())) return DICP_ERR_SHAPE;          // the scale must be a finite non-zero number of T
    if (n > (1 << 30) || m > (1 << 30)) return DICP_ERR_SHAPE;                                // row numbers are int32
    const size_t nch = (size_t)(D + SB_CH - 1) / SB_CH;
    if ((size_t)N * ((size_t)(n + SM_QUERIES - 1) / SM_QUERIES) * nch >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;   // the grids
    if ((size_t)N * ((size_t)(m + SM_QUERIES - 1) / SM_QUERIES) * nch >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;
    if (!fits62((size_t)N * n, 8, (size_t)D) || !fits62((size_t)N * m, 8, (size_t)D)) return DICP_ERR_SHAPE;
    return 0;
}

template <int CC>
void launch_soft_mfma(int np, unsigned grid, hipStream_t st, const float* x, const int32_t* x_rows, int n, const float* y, const float* h, const float* values,
                      const int32_t* y_rows, int m, int D, int C, int bpc, float c, float* out, float* lse, int64_t* idx, float* prob) {
    if (np <= 16) soft_mfma_kernel<16, CC><<<grid, BLOCK, 0, st>>>(x, x_rows, n, y, h, values, y_rows, m, D, C, bpc, c, out, lse, idx, prob);
    else if (np <= 32) soft_mfma_kernel<32, CC><<<grid, BLOCK, 0, st>>>(x, x_rows, n, y, h, values, y_rows, m, D, C, bpc, c, out, lse, idx, prob);
    else if (np <= 64) soft_mfma_kernel<64, CC><<<grid, BLOCK, 0, st>>>(x, x_rows, n, y, h, values, y_rows, m, D, C, bpc, c, out, lse, idx, prob);
    else soft_mfma_kernel<128, CC><<<grid, BLOCK, 0, st>>>(x, x_rows, n, y, h, values, y_rows, m, D, C, bpc, c, out, lse, idx, prob);
}

template <int CC, bool OWN_Y>
void launch_soft_bwd_mfma(int np, unsigned grid, hipStream_t st, const float* x, const int32_t* x_rows, int n, const float* y, const float* h, const float* values,
                          const int32_t* y_rows, int m, int D, int C, int bpc, float c, const float* out, const float* lse, const float* g, float* gown,
                          float* gv) {
    if (np <= 16) soft_bwd_mfma_kernel<16, CC, OWN_Y><<<grid, BLOCK, 0, st>>>(x, x_rows, n, y, h, values, y_rows, m, D, C, bpc, c, out, lse, g, gown, gv);
    else if (np <= 32) soft_bwd_mfma_kernel<32, CC, OWN_Y><<<grid, BLOCK, 0, st>>>(x, x_rows, n, y, h, values, y_rows, m, D, C, bpc, c, out, lse, g, gown, gv);
    else soft_bwd_mfma_kernel<64, CC, OWN_Y><<<grid, BLOCK, 0, st>>>(x, x_rows, n, y, h, values, y_rows, m, D, C, bpc, c, out, lse, g, gown, gv);
}

// f(integral_constant<CC>) for the capacity CC >= C of the per-query sums
template <typename F>
inline void with_ccap(int C, F&& f) {
    if (C <= 4) f(std::integral_constant<int, 4>());
    else f(std::integral_constant<int, SOFT_C_MAX>());
}

}  // namespace

size_t dicp_soft_match_workspace_bytes(int dtype, int N, int m) {
    if (bad_dtype(dtype) || N < 1 || m < 1) return 0;
    return up256((size_t)N * m * elem_size(dtype));
}

int dicp_soft_match(int dtype, const void* x, const int32_t* x_rows, int n, const void* y, const int32_t* y_rows, int m, int D, int N,
                    const void* values, int C, double tau, int form, void* out, void* lse, int64_t* idx, void* prob, void* workspace,
                    size_t workspace_bytes, void* stream) {
    if (!x || !y || !values || !out || !lse || !idx || !prob || !workspace) return DICP_ERR_NULL;
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (form != MATCH_FORM_AUTO && form != MATCH_FORM_VALU && form != MATCH_FORM_MFMA) return DICP_ERR_ENUM;
    if (form == MATCH_FORM_MFMA && dtype != DICP_F32) return DICP_ERR_ENUM;
    if (const int bad = soft_check(dtype, N, n, m, D, C, tau)) return bad;
    if (workspace_bytes < dicp_soft_match_workspace_bytes(dtype, N, m)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(x, ts) || misaligned(y, ts) || misaligned(values, ts) || misaligned(out, ts) || misaligned(lse, ts) || misaligned(prob, ts) ||
        misaligned(idx, 8) || misaligned(x_rows, 4) || misaligned(y_rows, 4) || misaligned(workspace, 16)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const bool mfma = dtype == DICP_F32 && form != MATCH_FORM_VALU;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        soft_norm_kernel<T><<<grid_1d((size_t)N * m), BLOCK, 0, st>>>((const T*)y, D, (size_t)N * m, (T*)workspace);
    });
    if (mfma) {
        const int bpc = (n + SM_QUERIES - 1) / SM_QUERIES;
        with_ccap(C, [&](auto cc) {
            launch_soft_mfma<decltype(cc)::value>((D + 1) / 2, (unsigned)N * (unsigned)bpc, st, (const float*)x, x_rows, n, (const float*)y,
                                                  (const float*)workspace, (const float*)values, y_rows, m, D, C, bpc, soft_scale<float>(tau), (float*)out,
                                                  (float*)lse, idx, (float*)prob);
        });
    } else {
        const int bpc = (n + BLOCK - 1) / BLOCK;
        with_scalar(dtype, [&](auto t) {
            using T = decltype(t);
            with_ccap(C, [&](auto cc) {
                soft_valu_kernel<T, decltype(cc)::value><<<(unsigned)N * (unsigned)bpc, BLOCK, 0, st>>>(
                    (const T*)x, x_rows, n, (const T*)y, (const T*)workspace, (const T*)values, y_rows, m, D, C, bpc, soft_scale<T>(tau), (T*)out, (T*)lse, idx,
                    (T*)prob);
            });
        });
    }
    return launch_status();
}

int dicp_soft_match_backward(int dtype, const void* x, const int32_t* x_rows, int n, const void* y, const int32_t* y_rows, int m, int D, int N,
                             const void* values, int C, double tau, int form, const void* out, const void* lse, const void* grad_out, void* grad_x,
                             void* grad_y, void* grad_values, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !y || !values || !out || !lse || !grad_out || !workspace) return DICP_ERR_NULL;
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (form != MATCH_FORM_AUTO && form != MATCH_FORM_VALU && form != MATCH_FORM_MFMA) return DICP_ERR_ENUM;
    if (form == MATCH_FORM_MFMA && (dtype != DICP_F32 || D > SOFT_BWD_MFMA_D)) return DICP_ERR_ENUM;
    if (const int bad = soft_check(dtype, N, n, m, D, C, tau)) return bad;
    if (workspace_bytes < dicp_soft_match_workspace_bytes(dtype, N, m)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(x, ts) || misaligned(y, ts) || misaligned(values, ts) || misaligned(out, ts) || misaligned(lse, ts) || misaligned(grad_out, ts) ||
        misaligned(grad_x, ts) || misaligned(grad_y, ts) || misaligned(grad_values, ts) || misaligned(x_rows, 4) || misaligned(y_rows, 4) ||
        misaligned(workspace, 16)) return DICP_ERR_ALIGN;
    if (!grad_x && !grad_y && !grad_values) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int nch = (D + SB_CH - 1) / SB_CH;
    begin_launch();
    if (dtype == DICP_F32 && form != MATCH_FORM_VALU && D <= SOFT_BWD_MFMA_D) {
        const float c = soft_scale<float>(tau);
        const float *fx = (const float*)x, *fy = (const float*)y, *hw = (const float*)workspace, *fv = (const float*)values;
        soft_norm_kernel<float><<<grid_1d((size_t)N * m), BLOCK, 0, st>>>(fy, D, (size_t)N * m, (float*)workspace);
        with_ccap(C, [&](auto cc) {
            constexpr int CC = decltype(cc)::value;
            if (grad_x) {
                const int bpc = (n + SM_QUERIES - 1) / SM_QUERIES;
                launch_soft_bwd_mfma<CC, false>((D + 1) / 2, (unsigned)N * (unsigned)bpc, st, fx, x_rows, n, fy, hw, fv, y_rows, m, D, C, bpc, c, (const float*)out,
                                                (const float*)lse, (const float*)grad_out, (float*)grad_x, nullptr);
            }
            if (grad_y || grad_values) {
                const int bpc = (m + SM_QUERIES - 1) / SM_QUERIES;
                launch_soft_bwd_mfma<CC, true>((D + 1) / 2, (unsigned)N * (unsigned)bpc, st, fx, x_rows, n, fy, hw, fv, y_rows, m, D, C, bpc, c, (const float*)out,
                                               (const float*)lse, (const float*)grad_out, (float*)grad_y, (float*)grad_values);
            }
        });
        return launch_status();
    }
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        const T c = soft_scale<T>(tau);
        soft_norm_kernel<T><<<grid_1d((size_t)N * m), BLOCK, 0, st>>>((const T*)y, D, (size_t)N * m, (T*)workspace);
        with_ccap(C, [&](auto cc) {
            constexpr int CC = decltype(cc)::value;
            if (grad_x) {
                const int bpc = (n + BLOCK - 1) / BLOCK;
                soft_bwd_q_kernel<T, CC><<<(unsigned)N * (unsigned)bpc * (unsigned)nch, BLOCK, 0, st>>>(
                    (const T*)x, x_rows, n, (const T*)y, (const T*)workspace, (const T*)values, y_rows, m, D, C, bpc, nch, c, (const T*)out, (const T*)lse,
                    (const T*)grad_out, (T*)grad_x);
            }
            if (grad_y || grad_values) {
                const int bpc = (m + BLOCK - 1) / BLOCK;
                // without grad_y one chunk does: it owns gvalues
                const int nc = grad_y ? nch : 1;
                soft_bwd_t_kernel<T, CC><<<(unsigned)N * (unsigned)bpc * (unsigned)nc, BLOCK, 0, st>>>(
                    (const T*)x, x_rows, n, (const T*)y, (const T*)workspace, (const T*)values, y_rows, m, D, C, bpc, nc, c, (const T*)out, (const T*)lse,
                    (const T*)grad_out, (T*)grad_y, (T*)grad_values);
            }
        });
    });
    return launch_status();
}
