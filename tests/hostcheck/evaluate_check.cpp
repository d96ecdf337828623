// TEST-ONLY host build of dicp_amd/csrc/dicp_evaluate.h (g++, no GPU): the query transform, the best-of-one scan, the ten terms, the tile
// tree and the join of the tiles -- the lines the HIP kernels execute -- run in a serial loop over a grid built on the host (as
// ball_check.cpp builds it), for tests/test_evaluate_host.py and tests/test_gpu_evaluate.py.  Never loaded by dicp_amd.
#include <algorithm>
#include <vector>

#include "../../dicp_amd/csrc/dicp_evaluate.h"

using namespace dicp;

namespace {

template <typename T> struct Row { T x, y, z; };

// dicp_evaluate_poses for one cloud: x (n, cx) with nb rows taking part, y (m, cy) with mb, poses (H, 4, 4)
// -> idx (H, n), d2 (H, n), counts (H), sums (H, 10), fitness (H), rmse (H); stats: [0] enlarged, [1] flat, [2] live rows, [3] rows visited
template <typename T>
void run(const T* x, int n, int cx, int nb, const T* y, int m, int cy, int mb, const T* poses, int H, T radius, int64_t* idx, T* d2, int32_t* counts,
         double* sums, double* fitness, double* rmse, int64_t* stats) {
    T mn[3], mx[3];
    int cnt = 0;
    std::vector<int> live;
    for (int j = 0; j < mb && j < m; ++j) {
        const T* p = y + (size_t)j * cy;
        if (!(ball_finite(p[0]) && ball_finite(p[1]) && ball_finite(p[2]))) continue;
        for (int d = 0; d < 3; ++d) {
            mn[d] = cnt ? std::min(mn[d], p[d]) : p[d];
            mx[d] = cnt ? std::max(mx[d], p[d]) : p[d];
        }
        ++cnt;
        live.push_back(j);
    }
    const BallPlan<T> P = ball_plan<T>(mn, mx, cnt, radius);
    std::vector<std::pair<uint64_t, int>> order;
    if (P.cnt) for (int j : live) order.push_back({ball_point_key(P, y[(size_t)j * cy], y[(size_t)j * cy + 1], y[(size_t)j * cy + 2]), j});
    std::sort(order.begin(), order.end());
    std::vector<Row<T>> rows4(order.size());
    for (size_t s = 0; s < order.size(); ++s) {
        const T* p = y + (size_t)order[s].second * cy;
        rows4[s] = {p[0], p[1], p[2]};
    }
    stats[0] = P.cnt && ball_enlarged(P);
    stats[1] = P.cnt && P.flat;
    stats[2] = P.cnt;
    stats[3] = 0;
    const int tiles = eval_tiles(n);
    std::vector<double> tile((size_t)EVAL_TILE * EVAL_TERMS), rec((size_t)std::max(tiles, 1) * EVAL_TERMS);
    auto keys = [&](int j) -> uint64_t { return order[j].first; };
    auto row = [&](int j) -> const Row<T>& { return rows4[j]; };
    auto orig = [&](int j) -> int { return order[j].second; };
    for (int h = 0; h < H; ++h) {
        T pose[12];
        eval_load_pose<T>(poses + (size_t)h * 16, pose);
        int32_t count = 0;
        for (int c = 0; c < tiles; ++c) {
            for (int l = 0; l < EVAL_TILE; ++l) {
                const int i = c * EVAL_TILE + l;
                EvalBest<T> best;
                eval_best_init(best);
                Row<T> ym = {T(0), T(0), T(0)};
                if (i < nb && i < n) {
                    const T* xp = x + (size_t)i * cx;
                    EvalPoint<T> q;
                    if (eval_query<T>(pose, xp[0], xp[1], xp[2], q)) {
                        const auto ins = eval_inserter<T>(best, orig);
                        const BallScan r = ball_scan<T>(P, q, keys, row, ins);
                        stats[3] += r.visited;
                        if (best.slot >= 0) ym = rows4[best.slot];
                    }
                }
                const bool matched = best.idx >= 0;
                if (i < n) {
                    idx[(size_t)h * n + i] = matched ? best.idx : -1;
                    d2[(size_t)h * n + i] = matched ? best.d2 : static_cast<T>(__builtin_huge_val());
                }
                double v[EVAL_TERMS];
                eval_terms<T>(matched, best.d2, ym, v);
                for (int k = 0; k < EVAL_TERMS; ++k) tile[(size_t)l * EVAL_TERMS + k] = v[k];
                count += matched ? 1 : 0;
            }
            for (int k = 0; k < EVAL_TERMS; ++k) {
                eval_tile_tree(tile.data() + k, EVAL_TILE, EVAL_TERMS);
                rec[(size_t)c * EVAL_TERMS + k] = tile[k];
            }
        }
        for (int k = 0; k < EVAL_TERMS; ++k) sums[(size_t)h * EVAL_TERMS + k] = eval_join_tiles(rec.data() + k, tiles, EVAL_TERMS);
        counts[h] = count;
        fitness[h] = eval_fitness(count, std::min(std::max(nb, 0), n));
        rmse[h] = eval_rmse(sums[(size_t)h * EVAL_TERMS + EVAL_E], count);
    }
}

}  // namespace

extern "C" {

int ec_tile() { return EVAL_TILE; }
int ec_terms() { return EVAL_TERMS; }
int ec_h_max() { return EVAL_H_MAX; }
void ec_run_f32(const float* x, int n, int cx, int nb, const float* y, int m, int cy, int mb, const float* poses, int H, float radius, int64_t* idx,
                float* d2, int32_t* counts, double* sums, double* fitness, double* rmse, int64_t* stats) {
    run<float>(x, n, cx, nb, y, m, cy, mb, poses, H, radius, idx, d2, counts, sums, fitness, rmse, stats);
}
void ec_run_f64(const double* x, int n, int cx, int nb, const double* y, int m, int cy, int mb, const double* poses, int H, double radius, int64_t* idx,
                double* d2, int32_t* counts, double* sums, double* fitness, double* rmse, int64_t* stats) {
    run<double>(x, n, cx, nb, y, m, cy, mb, poses, H, radius, idx, d2, counts, sums, fitness, rmse, stats);
}

}
