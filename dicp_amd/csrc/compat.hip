// Spatial compatibility of correspondences (dicp_compat_scores, dicp_compat_rank; dicp_amd/match.py).  The rules per element are
// csrc/dicp_compat.h's.  The input is the PACKED pair list of every cloud -- (N, n, 6) rows (x[0:3], y[0:3]) with the cloud's P live pairs
// first (dicp_select_rows' output) -- and P (N).  The work is every (p, q) of a cloud's pairs, P^2 per pass, never stored.
//
//   compat_pass_kernel   the hot path, run once per iteration: a lane per row p with its six values and the running sum w_p in registers;
//                        a workgroup takes BLOCK rows of one cloud and walks the cloud's packed rows q in ascending tiles of CP_TILE staged
//                        in LDS as a structure of arrays (x, y, v_q).  Every lane reads the same q (a broadcast read: no bank conflict), so
//                        the sum of a row is sequential in ascending q, as the definition has it.  Per (p, q): 6 subtractions, 6 fma, two
//                        square roots, a subtraction, four compares and a conditional add.  v_q = w_q / wmax of the previous pass is
//                        formed while the tile is loaded; the first pass has v = 1 and also writes the int32 degree.  The maximum of the
//                        pass is an integer atomic max on the bits of the (non-negative) sums: order-independent, so bit-reproducible.
//                        The grid is N x ceil(n / BLOCK) (never sized by P: nothing is read back); workgroups past P leave at once.
//                        Bound by the vector issue rate.
//   compat_finish_kernel score_p = w_p / wmax of the last pass (1 for iterations = 0) below P, 0 at and past it; the degree zeroed past P.
//   compat_rank_kernel   the same tile loop over the packed scores alone: rank_p = #{q : score_q > score_p, or equal and q < p}.
// No float atomics anywhere: every output is bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_compat.h"

namespace {

constexpr int CP_TILE = 512;            // packed rows q per LDS tile
constexpr int CP_NW = BLOCK / WAVE;

template <typename T> struct CpBits;
template <> struct CpBits<float>  { using type = unsigned int; };
template <> struct CpBits<double> { using type = unsigned long long; };

__device__ __forceinline__ unsigned int       cp_bits(float v)  { return __float_as_uint(v); }
__device__ __forceinline__ unsigned long long cp_bits(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ float  cp_value(unsigned int b)       { return __uint_as_float(b); }
__device__ __forceinline__ double cp_value(unsigned long long b) { return __longlong_as_double((long long)b); }

template <typename T, bool FIRST>
__global__ __launch_bounds__(BLOCK) void compat_pass_kernel(const T* __restrict__ pairs, const int32_t* __restrict__ P, const T* __restrict__ win,
                                                            const typename CpBits<T>::type* __restrict__ wmax_in, int n, int bpc, T thr, T L,
                                                            T* __restrict__ wout, typename CpBits<T>::type* __restrict__ wmax_out,
                                                            int32_t* __restrict__ degree) {
    __shared__ T sx[3][CP_TILE], sy[3][CP_TILE], sv[CP_TILE];
    __shared__ T smax[CP_NW];
    const int cloud = blockIdx.x / bpc, blk = blockIdx.x - cloud * bpc;
    const int Pc = min(max(P[cloud], 0), n);
    if (blk * BLOCK >= Pc) return;                          // (block-uniform)
    const int p = blk * BLOCK + (int)threadIdx.x;
    const bool live = p < Pc;
    const T* base = pairs + (size_t)cloud * n * COMPAT_ROW;
    T r[COMPAT_ROW];
#pragma unroll
    for (int k = 0; k < COMPAT_ROW; ++k) r[k] = live ? base[(size_t)p * COMPAT_ROW + k] : T(0);
    T wm = T(1);
    if (!FIRST) wm = cp_value(wmax_in[cloud]);
    T w = T(0);
    int deg = 0;
    for (int q0 = 0; q0 < Pc; q0 += CP_TILE) {
        const int len = min(CP_TILE, Pc - q0);
        __syncthreads();                                    // the previous tile has been read
        for (int j = threadIdx.x; j < len; j += BLOCK) {
            const T* row = base + (size_t)(q0 + j) * COMPAT_ROW;
            sx[0][j] = row[0]; sx[1][j] = row[1]; sx[2][j] = row[2];
            sy[0][j] = row[3]; sy[1][j] = row[4]; sy[2][j] = row[5];
            sv[j] = FIRST ? T(1) : compat_div<T>(win[(size_t)cloud * n + q0 + j], wm);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < len; ++j) {
            const bool ok = compat_pair<T>(r[0], r[1], r[2], r[3], r[4], r[5], sx[0][j], sx[1][j], sx[2][j], sy[0][j], sy[1][j], sy[2][j], thr, L);
            const bool same = q0 + j == p;
            w = w + compat_term<T>(same, ok, sv[j]);
            if (FIRST) deg += (ok && !same) ? 1 : 0;
        }
    }
    if (live) {
        wout[(size_t)cloud * n + p] = w;
        if (FIRST) degree[(size_t)cloud * n + p] = deg;
    }
    T mx = live ? w : T(0);
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) mx = max_t(mx, __shfl_xor(mx, off));
    if ((threadIdx.x & (WAVE - 1)) == 0) smax[threadIdx.x / WAVE] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < CP_NW; ++k) mx = max_t(mx, smax[k]);
        atomicMax(wmax_out + cloud, cp_bits(mx));           // non-negative values: the order of the bits is the order of the numbers
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void compat_finish_kernel(const T* __restrict__ w, const typename CpBits<T>::type* __restrict__ wmax,
                                                              const int32_t* __restrict__ P, int n, size_t total, int iterations,
                                                              T* __restrict__ score, int32_t* __restrict__ degree) {
    for (size_t e = (size_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (size_t)gridDim.x * BLOCK) {
        const int cloud = (int)(e / n), p = (int)(e - (size_t)cloud * n);
        const bool live = p < min(max(P[cloud], 0), n);
        T s = T(0);
        if (live) s = iterations == 0 ? T(1) : compat_div<T>(w[e], cp_value(wmax[cloud]));
        score[e] = s;
        if (!live) degree[e] = 0;
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void compat_rank_kernel(const T* __restrict__ score, const int32_t* __restrict__ P, int n, int bpc,
                                                            int32_t* __restrict__ rank) {
    __shared__ T ss[CP_TILE];
    const int cloud = blockIdx.x / bpc, blk = blockIdx.x - cloud * bpc;
    const int Pc = min(max(P[cloud], 0), n);
    const int p = blk * BLOCK + (int)threadIdx.x;
    if (blk * BLOCK >= Pc) {                                // (block-uniform) no pair here: a rank past every keep
        if (p < n) rank[(size_t)cloud * n + p] = 0x7fffffff;
        return;
    }
    const bool live = p < Pc;
    const T* sc = score + (size_t)cloud * n;
    const T sp = live ? sc[p] : T(0);
    int rk = 0;
    for (int q0 = 0; q0 < Pc; q0 += CP_TILE) {
        const int len = min(CP_TILE, Pc - q0);
        __syncthreads();
        for (int j = threadIdx.x; j < len; j += BLOCK) ss[j] = sc[q0 + j];
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < len; ++j) rk += compat_before<T>(ss[j], q0 + j, sp, p) ? 1 : 0;
    }
    if (p < n) rank[(size_t)cloud * n + p] = live ? rk : 0x7fffffff;
}

inline int compat_check(int dtype, int N, int n) {
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (N < 1 || n < 1 || n > (1 << 30)) return DICP_ERR_SHAPE;
    if ((size_t)N * ((size_t)(n + BLOCK - 1) / BLOCK) >= ((size_t)1 << 31) || (size_t)N * n >= ((size_t)1 << 40)) return DICP_ERR_SHAPE;     // the grids
    return 0;
}

}  // namespace

void dicp_compat_geometry(int* rows, int* tile) {
    if (rows) *rows = BLOCK;
    if (tile) *tile = CP_TILE;
}

int dicp_compat_scores(int dtype, const void* pairs, const int32_t* P, int N, int n, int iterations, double threshold, double min_length, void* w,
                       void* wmax, void* score, int32_t* degree, void* stream) {
    if (!pairs || !P || !w || !wmax || !score || !degree) return DICP_ERR_NULL;
    if (const int bad = compat_check(dtype, N, n)) return bad;
    if (iterations < 0 || iterations > COMPAT_ITER_MAX) return DICP_ERR_SHAPE;
    if (!(threshold > 0.0 && threshold < HUGE_VAL) || !(min_length >= 0.0 && min_length < HUGE_VAL)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(pairs, ts) || misaligned(w, ts) || misaligned(wmax, ts) || misaligned(score, ts) || misaligned(P, 4) || misaligned(degree, 4))
        return DICP_ERR_ALIGN;
    const int bpc = (n + BLOCK - 1) / BLOCK;
    const unsigned grid = (unsigned)N * (unsigned)bpc;
    const size_t total = (size_t)N * n;
    hipStream_t st = (hipStream_t)stream;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        using B = typename CpBits<T>::type;
        const T thr = compat_thr<T>(threshold), L = compat_thr<T>(min_length);
        T* wb[2] = {(T*)w, (T*)w + total};
        B* mx = (B*)wmax;
        compat_pass_kernel<T, true><<<grid, BLOCK, 0, st>>>((const T*)pairs, P, nullptr, nullptr, n, bpc, thr, L, wb[0], mx, degree);
        for (int it = 1; it < iterations; ++it)
            compat_pass_kernel<T, false><<<grid, BLOCK, 0, st>>>((const T*)pairs, P, wb[(it - 1) & 1], mx + (size_t)(it - 1) * N, n, bpc, thr, L, wb[it & 1],
                                                                 mx + (size_t)it * N, nullptr);
        const int last = iterations > 0 ? iterations - 1 : 0;
        compat_finish_kernel<T><<<grid_1d(total), BLOCK, 0, st>>>(wb[last & 1], mx + (size_t)last * N, P, n, total, iterations, (T*)score, degree);
    });
    return launch_status();
}

int dicp_compat_rank(int dtype, const void* score, const int32_t* P, int N, int n, int32_t* rank, void* stream) {
    if (!score || !P || !rank) return DICP_ERR_NULL;
    if (const int bad = compat_check(dtype, N, n)) return bad;
    if (misaligned(score, elem_size(dtype)) || misaligned(P, 4) || misaligned(rank, 4)) return DICP_ERR_ALIGN;
    const int bpc = (n + BLOCK - 1) / BLOCK;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        compat_rank_kernel<T><<<(unsigned)N * (unsigned)bpc, BLOCK, 0, (hipStream_t)stream>>>((const T*)score, P, n, bpc, rank);
    });
    return launch_status();
}
