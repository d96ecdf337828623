// RANSAC over explicit correspondences (dicp_ransac_hypotheses, dicp_ransac_score, dicp_ransac_best, dicp_pair_residuals;
// dicp_amd/match.py).  The rules per element are csrc/dicp_ransac.h's.  The input of the first three is the PACKED pair list of every
// cloud -- (N, n, 6) rows (x[0:3], y[0:3]) with the cloud's P live pairs first (dicp_select_rows' output) -- and P (N).
//
//   ransac_hyp_kernel    a lane per (cloud, hypothesis): the sample from the hash, three gathered rows, the 18 sums and kabsch_forward in
//                        double (one lane's 3x3 Jacobi SVD), the pose rounded to T.  Bound by the double-precision SVD; H lanes per cloud.
//   ransac_score_kernel  the hot path: a lane per hypothesis with the pose in 12 registers; a workgroup takes BLOCK hypotheses x a slice of
//                        RS_SLICE packed pairs of one cloud.  The slice is staged in LDS once and every lane walks it at the same address
//                        (a broadcast read: no bank conflict), 9 + 3 fma, 3 subtractions, a compare and a conditional add per (hypothesis,
//                        pair).  A lane's int count of the slice is added to counts[cloud, h] with one integer atomic: the result does not
//                        depend on the order.  The grid is N x slices x hypothesis blocks, sized by n (never by P: nothing is read back);
//                        blocks whose slice starts at or past P leave at once.  Bound by the vector issue rate.
//   ransac_best_kernel   a block per cloud: the (count descending, h ascending) maximum over H, then the winner's pose.
//   pair_residual_kernel a lane per original row: liveness, the clamped gather of y, the residual under the cloud's one pose; +inf for a
//                        row that is not live.
// No float atomics anywhere: every output is bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_ransac.h"

namespace {

constexpr int RS_SLICE = 256;           // packed pairs per workgroup of the score kernel
constexpr int RS_NW = BLOCK / WAVE;

template <typename T>
__global__ __launch_bounds__(BLOCK) void ransac_hyp_kernel(const T* __restrict__ pairs, const int32_t* __restrict__ P, int n, int H, int bpc, uint32_t seed,
                                                           T* __restrict__ poses, int32_t* __restrict__ samples) {
    const int cloud = blockIdx.x / bpc, h = (blockIdx.x - cloud * bpc) * BLOCK + (int)threadIdx.x;
    if (h >= H) return;
    const int Pc = min(max(P[cloud], 0), n);
    const size_t o = (size_t)cloud * H + h;
    T pose[12];
    int32_t a = -1, b = -1, c = -1;
    if (Pc >= 3) {
        ransac_sample(seed, (uint32_t)cloud, (uint32_t)h, (uint32_t)Pc, a, b, c);
        const T* base = pairs + (size_t)cloud * n * RANSAC_ROW;
        T ra[RANSAC_ROW], rb[RANSAC_ROW], rc[RANSAC_ROW];
#pragma unroll
        for (int k = 0; k < RANSAC_ROW; ++k) {
            ra[k] = base[(size_t)a * RANSAC_ROW + k];
            rb[k] = base[(size_t)b * RANSAC_ROW + k];
            rc[k] = base[(size_t)c * RANSAC_ROW + k];
        }
        ransac_fit<T>(ra, rb, rc, pose);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) pose[k] = (k < 9 && k % 4 == 0) ? T(1) : T(0);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) poses[o * 12 + k] = pose[k];
    samples[o * 3] = a; samples[o * 3 + 1] = b; samples[o * 3 + 2] = c;
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void ransac_score_kernel(const T* __restrict__ pairs, const int32_t* __restrict__ P, const T* __restrict__ poses, int n,
                                                             int H, int hb, int spc, T thr2, int32_t* __restrict__ counts) {
    __shared__ T rows[RS_SLICE * RANSAC_ROW];
    const int hblk = blockIdx.x % hb, rest = blockIdx.x / hb;
    const int slice = rest % spc, cloud = rest / spc;
    const int Pc = min(max(P[cloud], 0), n);
    const int base = slice * RS_SLICE;
    if (Pc < 3 || base >= Pc) return;                       // (block-uniform)
    const int len = min(RS_SLICE, Pc - base);
    const T* src = pairs + ((size_t)cloud * n + base) * RANSAC_ROW;
    for (int e = threadIdx.x; e < len * RANSAC_ROW; e += BLOCK) rows[e] = src[e];
    __syncthreads();
    const int h = hblk * BLOCK + (int)threadIdx.x;
    if (h >= H) return;
    T pose[12];
    const T* ps = poses + ((size_t)cloud * H + h) * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = ps[k];
    int cnt = 0;
#pragma unroll 4
    for (int j = 0; j < len; ++j) {
        const T* r = rows + j * RANSAC_ROW;
        cnt += ransac_inlier<T>(ransac_residual<T>(pose, r[0], r[1], r[2], r[3], r[4], r[5]), thr2) ? 1 : 0;
    }
    if (cnt) atomicAdd(counts + (size_t)cloud * H + h, cnt);
}

__global__ __launch_bounds__(BLOCK) void ransac_best_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ P, int H, int32_t* __restrict__ best,
                                                            int32_t* __restrict__ best_count) {
    __shared__ int32_t wc[RS_NW], wh[RS_NW];
    const int cloud = blockIdx.x;
    const int32_t* cc = counts + (size_t)cloud * H;
    int32_t bc = -1, bh = 0x7fffffff;
    for (int h = threadIdx.x; h < H; h += BLOCK) {
        const int32_t c = cc[h];
        if (ransac_better(c, h, bc, bh)) { bc = c; bh = h; }
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const int32_t oc = __shfl_xor(bc, off), oh = __shfl_xor(bh, off);
        if (ransac_better(oc, oh, bc, bh)) { bc = oc; bh = oh; }
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) { wc[threadIdx.x / WAVE] = bc; wh[threadIdx.x / WAVE] = bh; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 1; q < RS_NW; ++q)
            if (ransac_better(wc[q], wh[q], bc, bh)) { bc = wc[q]; bh = wh[q]; }
        const bool none = P[cloud] < 3;
        best[cloud] = none ? -1 : bh;
        best_count[cloud] = none ? 0 : bc;
    }
}

// pose_best[cloud] = poses[cloud, best[cloud]], the identity for best < 0
template <typename T>
__global__ __launch_bounds__(BLOCK) void ransac_pose_kernel(const T* __restrict__ poses, const int32_t* __restrict__ best, int N, int H, T* __restrict__ pose_best) {
    for (size_t e = (size_t)blockIdx.x * BLOCK + threadIdx.x; e < (size_t)N * 12; e += (size_t)gridDim.x * BLOCK) {
        const size_t cloud = e / 12;
        const int k = (int)(e - cloud * 12);
        const int32_t h = best[cloud];
        pose_best[e] = (h >= 0 && h < H) ? poses[(cloud * H + h) * 12 + k] : ((k < 9 && k % 4 == 0) ? T(1) : T(0));
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void pair_residual_kernel(const T* __restrict__ x, const T* __restrict__ y, const int32_t* __restrict__ idx,
                                                              const int32_t* __restrict__ x_rows, const T* __restrict__ pose, int n, int m, size_t total,
                                                              T* __restrict__ d2) {
    for (size_t q = (size_t)blockIdx.x * BLOCK + threadIdx.x; q < total; q += (size_t)gridDim.x * BLOCK) {
        const int cloud = (int)(q / n), i = (int)(q - (size_t)cloud * n);
        const int32_t j0 = idx[q];
        const int j = min(max(j0, 0), m - 1);
        const T* xr = x + q * 3;
        const T* yr = y + ((size_t)cloud * m + j) * 3;
        const T xv[3] = {xr[0], xr[1], xr[2]}, yv[3] = {yr[0], yr[1], yr[2]};
        T d = inf_v<T>();
        if (ransac_live<T>(i < rows_of(x_rows, cloud, n), (int64_t)j0, xv, yv)) {
            T ps[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) ps[k] = pose[(size_t)cloud * 12 + k];
            d = ransac_residual<T>(ps, xv[0], xv[1], xv[2], yv[0], yv[1], yv[2]);
        }
        d2[q] = d;
    }
}

inline int ransac_check(int dtype, int N, int n, int H) {
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (N < 1 || n < 1 || H < 1 || H > RANSAC_H_MAX || n > (1 << 30)) return DICP_ERR_SHAPE;
    const size_t hb = (size_t)(H + BLOCK - 1) / BLOCK, spc = (size_t)(n + RS_SLICE - 1) / RS_SLICE;
    if ((size_t)N * hb * spc >= ((size_t)1 << 31) || (size_t)N * H * 12 >= ((size_t)1 << 40)) return DICP_ERR_SHAPE;    // the grids
    return 0;
}

}  // namespace

int dicp_ransac_slice(void) { return RS_SLICE; }

int dicp_ransac_hypotheses(int dtype, const void* pairs, const int32_t* P, int N, int n, int H, uint32_t seed, void* poses, int32_t* samples,
                           void* stream) {
    if (!pairs || !P || !poses || !samples) return DICP_ERR_NULL;
    if (const int bad = ransac_check(dtype, N, n, H)) return bad;
    const size_t ts = elem_size(dtype);
    if (misaligned(pairs, ts) || misaligned(poses, ts) || misaligned(P, 4) || misaligned(samples, 4)) return DICP_ERR_ALIGN;
    const int bpc = (H + BLOCK - 1) / BLOCK;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        ransac_hyp_kernel<T><<<(unsigned)N * (unsigned)bpc, BLOCK, 0, (hipStream_t)stream>>>((const T*)pairs, P, n, H, bpc, seed, (T*)poses, samples);
    });
    return launch_status();
}

int dicp_ransac_score(int dtype, const void* pairs, const int32_t* P, const void* poses, int N, int n, int H, double threshold, int32_t* counts,
                      void* stream) {
    if (!pairs || !P || !poses || !counts) return DICP_ERR_NULL;
    if (const int bad = ransac_check(dtype, N, n, H)) return bad;
    if (!(threshold > 0.0 && threshold < HUGE_VAL)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(pairs, ts) || misaligned(poses, ts) || misaligned(P, 4) || misaligned(counts, 4)) return DICP_ERR_ALIGN;
    const int hb = (H + BLOCK - 1) / BLOCK, spc = (n + RS_SLICE - 1) / RS_SLICE;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        ransac_score_kernel<T><<<(unsigned)N * (unsigned)spc * (unsigned)hb, BLOCK, 0, (hipStream_t)stream>>>((const T*)pairs, P, (const T*)poses, n, H, hb, spc,
                                                                                                            ransac_thr2<T>(threshold), counts);
    });
    return launch_status();
}

int dicp_ransac_best(int dtype, const int32_t* counts, const void* poses, const int32_t* P, int N, int H, int32_t* best, int32_t* best_count,
                     void* pose_best, void* stream) {
    if (!counts || !poses || !P || !best || !best_count || !pose_best) return DICP_ERR_NULL;
    if (const int bad = ransac_check(dtype, N, 1, H)) return bad;
    const size_t ts = elem_size(dtype);
    if (misaligned(poses, ts) || misaligned(pose_best, ts) || misaligned(counts, 4) || misaligned(P, 4) || misaligned(best, 4) || misaligned(best_count, 4))
        return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    begin_launch();
    ransac_best_kernel<<<(unsigned)N, BLOCK, 0, st>>>(counts, P, H, best, best_count);
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        ransac_pose_kernel<T><<<grid_1d((size_t)N * 12), BLOCK, 0, st>>>((const T*)poses, best, N, H, (T*)pose_best);
    });
    return launch_status();
}

int dicp_pair_residuals(int dtype, const void* x, const void* y, const int32_t* idx, const int32_t* x_rows, const void* pose, int N, int n, int m,
                        void* d2, void* stream) {
    if (!x || !y || !idx || !pose || !d2) return DICP_ERR_NULL;
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (N < 1 || n < 1 || m < 1 || n > (1 << 30) || m > (1 << 30) || (size_t)N * n >= ((size_t)1 << 40)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(x, ts) || misaligned(y, ts) || misaligned(pose, ts) || misaligned(d2, ts) || misaligned(idx, 4) || misaligned(x_rows, 4)) return DICP_ERR_ALIGN;
    const size_t total = (size_t)N * n;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        pair_residual_kernel<T><<<grid_1d(total), BLOCK, 0, (hipStream_t)stream>>>((const T*)x, (const T*)y, idx, x_rows, (const T*)pose, n, m, total, (T*)d2);
    });
    return launch_status();
}
