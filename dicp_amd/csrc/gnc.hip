// Graduated non-convexity over explicit correspondences (dicp_gnc_fit; dicp_amd/match.py: gnc_correspondences).  The rules per element,
// the order of the sums and the stopping rules are csrc/dicp_gnc.h's.  The input is the PACKED pair list of every cloud -- (N, n, 6) rows
// (x[0:3], y[0:3]) with the cloud's P live pairs first (dicp_select_rows' output) --, P (N) and optionally the packed user weights (N, n).
//
//   gnc_kernel   ONE launch, one workgroup of GNC_SLOTS = 1024 lanes per cloud, every round inside it.  A pass: lane s walks its pairs
//                p = s, s + 1024, ... (re-read from L2 every round: 24 / 48 bytes per pair), residual, weight and the 18 weighted
//                products in double; the sums, the count of pairs that still carry weight and the band count are reduced by a butterfly
//                over the wave's lanes and 16 records in LDS; lane k < 18 adds the records of sum k in the header's tree; lane 0 takes
//                the stopping decision (gnc_apply), runs kabsch_forward (one lane's 3x3 Jacobi SVD in double) and publishes pose, next
//                mu and the decision in LDS.  Three barriers per pass, none under a lane-dependent condition; the trip count is bounded
//                by `iterations`.
//                Round 0 takes two passes (the fit at weight 1, then the largest residual), every later round one, and a last pass
//                writes the weights of the last applied round.  Bound by the serial fit of lane 0 and the barriers for small
//                P, by the double-precision products of the pass for large P (profiles/r32_gnc_bench.txt).
// No float atomics, nothing read back: every output is bit-reproducible.
//
// Contraction is off for the whole translation unit: kabsch_forward and svd3 (dicp_math.h) then round every product and sum on their own,
// as the g++ build of the header does, and the kernel's poses equal that build's bit for bit.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_gnc.h"

namespace {

constexpr int GNC_NW = GNC_SLOTS / WAVE;

struct GncShared {
    double part[GNC_NW][NKAB];
    double sums[NKAB];                  // the tree's totals
    double dmax[GNC_NW];
    long long npos[GNC_NW], band[GNC_NW];
    double pose[12];                    // the current pose
    double pose_w[12];                  // the pose whose residuals gave the weights of the last applied round
    GncRound rd, rd_used;               // of the next round / of the last applied round
    GncState st;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) v = v + __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

// the levels of the tree above a wave: lane k < 18 adds the 16 waves' records of sum k in registers, in the header's order
__device__ __forceinline__ void gnc_join_records(GncShared& sh, int lane) {
    if (lane < NKAB) {
        double v[GNC_NW];
#pragma unroll
        for (int q = 0; q < GNC_NW; ++q) v[q] = sh.part[q][lane];
        gnc_tree_one(v, GNC_NW, 1);
        sh.sums[lane] = v[0];
    }
}

// lane 0's serial part of a pass, kept out of line so that its 3x3 SVD does not share registers with the loops over the pairs: the
// closed form of the totals; sh.pose_w takes the pose that was current, sh.pose the new one
__device__ __noinline__ void gnc_fit_sums(GncShared& sh) {
    double acc[NKAB], C[9], r[3], save[KAB_SAVE];
    for (int k = 0; k < NKAB; ++k) acc[k] = sh.sums[k];
    kabsch_forward(acc, C, r, save);
    for (int k = 0; k < 12; ++k) sh.pose_w[k] = sh.pose[k];
    for (int k = 0; k < 9; ++k) sh.pose[k] = C[k];
    for (int k = 0; k < 3; ++k) sh.pose[9 + k] = r[k];
}

template <typename T>
__global__ __launch_bounds__(GNC_SLOTS) void gnc_kernel(const T* __restrict__ pairs, const int32_t* __restrict__ P, const T* __restrict__ u, int n, int loss,
                                                        double c2, double growth, int iterations, T* __restrict__ weights, int32_t* __restrict__ rounds,
                                                        int32_t* __restrict__ status, double* __restrict__ mu, T* __restrict__ pose_last,
                                                        double* __restrict__ trace) {
    __shared__ GncShared sh;
    const int cloud = blockIdx.x, lane = threadIdx.x, wave = lane / WAVE;
    const bool leader = (lane & (WAVE - 1)) == 0;
    const int Pc = min(max(P[cloud], 0), n);
    const T* base = pairs + (size_t)cloud * n * GNC_ROW;
    const T* ub = u ? u + (size_t)cloud * n : nullptr;
    T* wout = weights + (size_t)cloud * n;
    double* tr = trace ? trace + (size_t)cloud * (iterations + 1) * GNC_TRACE : nullptr;
    if (Pc < 3) {                                                           // (block-uniform)
        for (int p = lane; p < n; p += GNC_SLOTS) wout[p] = T(0);
        if (lane == 0) {
            rounds[cloud] = 0; status[cloud] = GNC_TOO_FEW; mu[cloud] = 0.0;
#pragma unroll
            for (int k = 0; k < 12; ++k) pose_last[(size_t)cloud * 12 + k] = (k < 9 && k % 4 == 0) ? T(1) : T(0);
        }
        return;
    }
    // ---- round 0: the fit at w = 1, then the largest finite residual
    {
        double acc[NKAB];
#pragma unroll
        for (int k = 0; k < NKAB; ++k) acc[k] = 0.0;
        for (int p = lane; p < Pc; p += GNC_SLOTS) {
            const double omega = ub ? (double)ub[p] * 1.0 : 1.0;
            if (omega > 0.0) gnc_add<T>(acc, omega, base + (size_t)p * GNC_ROW);
        }
#pragma unroll
        for (int k = 0; k < NKAB; ++k) {
            const double v = wave_sum(acc[k]);
            if (leader) sh.part[wave][k] = v;
        }
    }
    __syncthreads();
    gnc_join_records(sh, lane);
    __syncthreads();
    if (lane == 0) {
        gnc_fit_sums(sh);
        for (int k = 0; k < 12; ++k) sh.pose_w[k] = sh.pose[k];
        if (tr) {
            tr[0] = 0.0; tr[1] = 0.0;
            for (int k = 0; k < NKAB; ++k) tr[2 + k] = sh.sums[k];
            for (int k = 0; k < 12; ++k) tr[2 + NKAB + k] = sh.pose[k];
        }
    }
    __syncthreads();
    {
        double pose[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) pose[k] = sh.pose[k];
        double dm = 0.0;
        for (int p = lane; p < Pc; p += GNC_SLOTS) {
            const double d = gnc_residual<T>(pose, base + (size_t)p * GNC_ROW);
            if (d < gnc_inf() && d > dm) dm = d;
        }
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const double o = __shfl_xor(dm, off);
            dm = o > dm ? o : dm;
        }
        if (leader) sh.dmax[wave] = dm;
    }
    __syncthreads();
    if (lane == 0) {
        double dm = sh.dmax[0];
#pragma unroll
        for (int q = 1; q < GNC_NW; ++q) dm = sh.dmax[q] > dm ? sh.dmax[q] : dm;
        GncState st;
        gnc_begin(loss, dm, c2, st);
        sh.st = st;
        sh.rd = sh.rd_used = gnc_round(loss, st.mu, c2);
    }
    __syncthreads();
    // ---- the rounds: the trip count is bounded by `iterations` whatever the data holds
    for (int it = 0; it < iterations; ++it) {
        if (!sh.st.go) break;                                               // (block-uniform: written before the last barrier)
        double pose[12], acc[NKAB];
#pragma unroll
        for (int k = 0; k < 12; ++k) pose[k] = sh.pose[k];
#pragma unroll
        for (int k = 0; k < NKAB; ++k) acc[k] = 0.0;
        const GncRound rd = sh.rd;
        long long npos = 0, nband = 0;
        for (int p = lane; p < Pc; p += GNC_SLOTS) {
            const T* row = base + (size_t)p * GNC_ROW;
            int b;
            const double w = gnc_weight(rd, gnc_residual<T>(pose, row), b);
            const double omega = ub ? (double)ub[p] * w : w;
            if (omega > 0.0) { gnc_add<T>(acc, omega, row); ++npos; }
            nband += b;
        }
#pragma unroll
        for (int k = 0; k < NKAB; ++k) {
            const double v = wave_sum(acc[k]);
            if (leader) sh.part[wave][k] = v;
        }
        npos = wave_sum(npos);
        nband = wave_sum(nband);
        if (leader) { sh.npos[wave] = npos; sh.band[wave] = nband; }
        __syncthreads();
        gnc_join_records(sh, lane);
        __syncthreads();
        if (lane == 0) {
            long long np = 0, nb = 0;
#pragma unroll
            for (int q = 0; q < GNC_NW; ++q) { np += sh.npos[q]; nb += sh.band[q]; }
            GncState st = sh.st;
            if (gnc_apply(loss, np, nb, growth, iterations, st)) {
                gnc_fit_sums(sh);
                sh.rd_used = sh.rd;
                if (tr) {
                    double* t = tr + (size_t)st.rounds * GNC_TRACE;
                    t[0] = st.mu_used; t[1] = (double)nb;
                    for (int k = 0; k < NKAB; ++k) t[2 + k] = sh.sums[k];
                    for (int k = 0; k < 12; ++k) t[2 + NKAB + k] = sh.pose[k];
                }
                if (st.go) sh.rd = gnc_round(loss, st.mu, c2);
            }
            sh.st = st;
        }
        __syncthreads();
    }
    // ---- the weights of the last applied round (w = 1 when none was), rounded once; 0 at and past P
    {
        const int applied = sh.st.rounds;
        double pose[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) pose[k] = sh.pose_w[k];
        const GncRound rd = sh.rd_used;
        for (int p = lane; p < n; p += GNC_SLOTS) {
            double w = 0.0;
            if (p < Pc) {
                int b;
                w = applied ? gnc_weight(rd, gnc_residual<T>(pose, base + (size_t)p * GNC_ROW), b) : 1.0;
            }
            wout[p] = (T)w;
        }
        if (lane == 0) {
            rounds[cloud] = sh.st.rounds; status[cloud] = sh.st.status; mu[cloud] = sh.st.mu_used;
#pragma unroll
            for (int k = 0; k < 12; ++k) pose_last[(size_t)cloud * 12 + k] = (T)sh.pose[k];
        }
    }
}

}  // namespace

int dicp_gnc_fit(int dtype, const void* pairs, const int32_t* P, const void* u, int N, int n, int loss, double threshold, double growth, int iterations,
                 void* weights_packed, int32_t* rounds, int32_t* status, double* mu, void* pose_last, double* trace, void* stream) {
    if (!pairs || !P || !weights_packed || !rounds || !status || !mu || !pose_last) return DICP_ERR_NULL;
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (loss != GNC_TLS && loss != GNC_GM) return DICP_ERR_ENUM;
    if (N < 1 || n < 1 || n > (1 << 30) || N > (1 << 20) || gnc_bad_arguments(loss, threshold, growth, iterations)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(pairs, ts) || misaligned(u, ts) || misaligned(weights_packed, ts) || misaligned(pose_last, ts) || misaligned(P, 4) || misaligned(rounds, 4) ||
        misaligned(status, 4) || misaligned(mu, 8) || misaligned(trace, 8))
        return DICP_ERR_ALIGN;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        gnc_kernel<T><<<(unsigned)N, GNC_SLOTS, 0, (hipStream_t)stream>>>((const T*)pairs, P, (const T*)u, n, loss, threshold * threshold, growth, iterations,
                                                                          (T*)weights_packed, rounds, status, mu, (T*)pose_last, trace);
    });
    return launch_status();
}
