// Registration quality of many candidate poses per cloud against ONE cell grid of the target (dicp_evaluate_poses; dicp_amd/evaluate.py:
// evaluate_registration, information_matrix).  The rules per row and the order of the sums are csrc/dicp_evaluate.h's; the grid is the
// one dicp_ball_grid_build makes (csrc/ball_query.hip), read here and never built.
//
//   evaluate_kernel   one workgroup of 256 lanes per (cloud, pose, tile of 256 source rows), one lane per row IN THE ORIGINAL ROW ORDER
//                     (the order of the sums is a function of the row index).  The pose's 12 values are loaded once (a uniform address:
//                     scalar loads), the lane transforms its row with the header's fma chain and runs ball_scan of csrc/dicp_ball.h with
//                     the best-of-one inserter -- the same candidates, the same d2 and the same (d2, index) order as dicp_ball_query at
//                     k = 1 --, gathers the matched row from the grid's packed rows and forms the ten double terms.  Terms and count are
//                     reduced by a butterfly over the wave's lanes (a + b is b + a bit for bit, so lane 0 holds the pairwise tree's
//                     value) and the four waves' records are joined through LDS, (w0 + w1) + (w2 + w3): the tree's last two levels.
//                     One record of ten doubles and one count per workgroup go to the workspace; idx and d2 are written per row where asked
//                     for.  The queries are NOT re-sorted by cell: a wave's locality rests on the caller's row order.
//   evaluate_finish   one lane per (cloud, pose, sum): the tiles' records in ascending order from +0; the lane of the count also writes
//                     fitness and rmse.
// No float atomics, no spin-waits, nothing read back; every loop is bounded by ball_scan's own bound (the target's row count) or by the
// number of tiles: every output is bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_evaluate.h"
#include "kernels_grid_plan.h"

namespace {

constexpr int EVAL_NW = EVAL_TILE / WAVE;
static_assert(EVAL_NW == 4, "the join of the waves' records is written out for four waves");

template <typename T>
__global__ __launch_bounds__(EVAL_TILE) void evaluate_kernel(const T* __restrict__ src, int c, const int32_t* __restrict__ src_rows, int n,
                                                             const T* __restrict__ poses, int H, int tiles, const void* __restrict__ plans,
                                                             const uint64_t* __restrict__ ykeys, const int32_t* __restrict__ yperm,
                                                             const typename V4<T>::type* __restrict__ yrows4, int Pm, double* __restrict__ rec,
                                                             int32_t* __restrict__ rec_count, int64_t* __restrict__ idx_out, T* __restrict__ d2_out) {
    using T4 = typename V4<T>::type;
    __shared__ double part[EVAL_NW][EVAL_TERMS];
    __shared__ int32_t pcount[EVAL_NW];
    const unsigned blk = blockIdx.x;
    const int tile = (int)(blk % (unsigned)tiles);
    const unsigned bh = blk / (unsigned)tiles;              // cloud * H + pose
    const int b = (int)(bh / (unsigned)H);
    const int lane = threadIdx.x;
    const int i = tile * EVAL_TILE + lane;
    T pose[12];
    eval_load_pose<T>(poses + (size_t)bh * 16, pose);
    const int nb = rows_of(src_rows, b, n);
    EvalBest<T> best;
    eval_best_init(best);
    T4 ym = {};
    if (i < nb) {
        const T* xp = src + ((size_t)b * n + i) * c;
        EvalPoint<T> q;
        if (eval_query<T>(pose, xp[0], xp[1], xp[2], q)) {
            const BallPlan<T> pl = plan_of<T>(plans, b);
            const size_t ybase = (size_t)b * Pm;
            const uint64_t* kb = ykeys + ybase;
            auto keys = [&](int j) -> uint64_t { return kb[j]; };
            auto row = [&](int j) -> T4 { return yrows4[ybase + j]; };
            auto orig = [&](int j) -> int { return yperm[ybase + j]; };
            const auto ins = eval_inserter<T>(best, orig);
            ball_scan<T>(pl, q, keys, row, ins);
            if (best.slot >= 0) ym = yrows4[ybase + best.slot];
        }
    }
    const bool matched = best.idx >= 0;
    if (i < n) {
        const size_t o = (size_t)bh * n + i;
        if (idx_out) idx_out[o] = matched ? (int64_t)best.idx : (int64_t)-1;
        if (d2_out) d2_out[o] = matched ? best.d2 : inf_v<T>();
    }
    double v[EVAL_TERMS];
    eval_terms<T>(matched, best.d2, ym, v);
    int32_t cnt = matched ? 1 : 0;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
#pragma unroll
        for (int k = 0; k < EVAL_TERMS; ++k) v[k] = v[k] + __shfl_xor(v[k], off);
        cnt += __shfl_xor(cnt, off);
    }
    const int wave = lane / WAVE;
    if ((lane & (WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < EVAL_TERMS; ++k) part[wave][k] = v[k];
        pcount[wave] = cnt;
    }
    __syncthreads();
    if (lane < EVAL_TERMS) {
        const double lo = part[0][lane] + part[1][lane];
        const double hi = part[2][lane] + part[3][lane];
        rec[(size_t)blk * EVAL_TERMS + lane] = lo + hi;
    } else if (lane == EVAL_TERMS) {
        rec_count[blk] = (pcount[0] + pcount[1]) + (pcount[2] + pcount[3]);
    }
}

__global__ __launch_bounds__(BLOCK) void evaluate_finish_kernel(const double* __restrict__ rec, const int32_t* __restrict__ rec_count,
                                                                const int32_t* __restrict__ src_rows, int n, int H, int tiles, size_t NH,
                                                                double* __restrict__ sums, int32_t* __restrict__ counts,
                                                                double* __restrict__ fitness, double* __restrict__ rmse) {
    const size_t e = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= NH * (EVAL_TERMS + 1)) return;
    const size_t bh = e / (EVAL_TERMS + 1);
    const int k = (int)(e - bh * (EVAL_TERMS + 1));
    const double* base = rec + bh * (size_t)tiles * EVAL_TERMS;
    if (k < EVAL_TERMS) {
        sums[bh * EVAL_TERMS + k] = eval_join_tiles(base + k, tiles, EVAL_TERMS);
        return;
    }
    const int32_t* cb = rec_count + bh * (size_t)tiles;
    int32_t cnt = 0;
    for (int t = 0; t < tiles; ++t) cnt += cb[t];
    counts[bh] = cnt;
    fitness[bh] = eval_fitness(cnt, rows_of(src_rows, (int)(bh / (size_t)H), n));
    rmse[bh] = eval_rmse(eval_join_tiles(base + EVAL_E, tiles, EVAL_TERMS), cnt);
}

// the workgroups of the forward launch, 0 where the arguments do not fit
inline size_t eval_groups(int N, int H, int n) {
    if (N < 1 || n < 1 || n > (1 << 30) || H < 1 || H > EVAL_H_MAX) return 0;
    const size_t g = (size_t)N * (size_t)H * (size_t)eval_tiles(n);
    return g < ((size_t)1 << 31) ? g : 0;
}
inline size_t eval_rec_bytes(size_t groups) { return up256(groups * EVAL_TERMS * sizeof(double)); }
inline size_t eval_ws_bytes(size_t groups) { return eval_rec_bytes(groups) + up256(groups * sizeof(int32_t)); }

}  // namespace

size_t dicp_evaluate_workspace_bytes(int N, int H, int n) {
    const size_t g = eval_groups(N, H, n);
    return g ? eval_ws_bytes(g) : 0;
}

int dicp_evaluate_poses(int dtype, const void* source, int c, const int32_t* source_rows, int n, const void* poses, int H, const void* y_plans,
                        const uint64_t* y_keys, const int32_t* y_perm, const void* y_rows4, int m, int N, void* workspace, size_t workspace_bytes,
                        double* sums, int32_t* counts, double* fitness, double* rmse, int64_t* idx, void* d2, void* stream) {
    if (!source || !poses || !y_plans || !y_keys || !y_perm || !y_rows4 || !workspace || !sums || !counts || !fitness || !rmse) return DICP_ERR_NULL;
    int rc = ball_check(dtype, N, n);
    if (rc || (rc = ball_check(dtype, N, m))) return rc;
    const size_t groups = eval_groups(N, H, n);
    if (c < 3 || !groups || workspace_bytes < eval_ws_bytes(groups)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(source, ts) || misaligned(source_rows, 4) || misaligned(poses, ts) || misaligned(y_plans, 8) || misaligned(y_keys, 8) ||
        misaligned(y_perm, 4) || misaligned(y_rows4, 4 * ts) || misaligned(workspace, 256) || misaligned(sums, 8) || misaligned(counts, 4) ||
        misaligned(fitness, 8) || misaligned(rmse, 8) || misaligned(idx, 8) || misaligned(d2, ts)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int tiles = eval_tiles(n), Pm = ball_slots(m);
    double* rec = (double*)workspace;
    int32_t* rec_count = (int32_t*)((char*)workspace + eval_rec_bytes(groups));
    const size_t NH = (size_t)N * H;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        evaluate_kernel<T><<<(unsigned)groups, EVAL_TILE, 0, st>>>((const T*)source, c, source_rows, n, (const T*)poses, H, tiles, y_plans, y_keys, y_perm,
                                                                   (const typename V4<T>::type*)y_rows4, Pm, rec, rec_count, idx, (T*)d2);
    });
    evaluate_finish_kernel<<<(unsigned)((NH * (EVAL_TERMS + 1) + BLOCK - 1) / BLOCK), BLOCK, 0, st>>>(rec, rec_count, source_rows, n, H, tiles, NH, sums,
                                                                                                    counts, fitness, rmse);
    return launch_status();
}
