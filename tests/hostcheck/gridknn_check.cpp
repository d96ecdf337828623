// TEST-ONLY host build of dicp_amd/csrc/dicp_gridknn.h (g++, no GPU): the density plan, the cell keys and the per-query k-NN scan that
// the HIP kernels execute, run serially on a grid built on the host, for tests/test_gridknn_host.py.  Never loaded by dicp_amd.
#include <algorithm>
#include <vector>

#include "../../dicp_amd/csrc/dicp_gridknn.h"

using namespace dicp;

namespace {

template <typename T> struct Row { T x, y, z; };

// stats: [0] edge enlarged, [1] flat, [2] rows visited, [3] live rows, [4] the most passes of a query, [5] queries with more than one
// growth pass, [6] queries whose closing pass fed a row, [7] queries that ended on the whole grid, [8] passes of all queries,
// [9] the header's bound on the passes of a query
template <typename T, int K>
void run(const T* x, int n, int cx, int nb, const T* y, int m, int cy, int mb, int k, T edge, T* d2, int64_t* idx, int64_t* stats) {
    T mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    int cnt = 0;
    std::vector<int> live;
    for (int j = 0; j < mb; ++j) {
        const T* p = y + (size_t)j * cy;
        if (!(ball_finite(p[0]) && ball_finite(p[1]) && ball_finite(p[2]))) continue;
        for (int d = 0; d < 3; ++d) {
            mn[d] = cnt ? std::min(mn[d], p[d]) : p[d];
            mx[d] = cnt ? std::max(mx[d], p[d]) : p[d];
        }
        ++cnt;
        live.push_back(j);
    }
    const BallPlan<T> P = edge > T(0) ? gknn_plan_at<T>(mn, mx, cnt, edge) : gknn_plan<T>(mn, mx, cnt);     // edge <= 0: the density rule
    std::vector<std::pair<uint64_t, int>> order;
    if (P.cnt) for (int j : live) order.push_back({ball_point_key(P, y[(size_t)j * cy], y[(size_t)j * cy + 1], y[(size_t)j * cy + 2]), j});
    std::sort(order.begin(), order.end());
    std::vector<Row<T>> rows4(order.size());
    for (size_t s = 0; s < order.size(); ++s) {
        const T* p = y + (size_t)order[s].second * cy;
        rows4[s] = {p[0], p[1], p[2]};
    }
    for (int i = 0; i < 10; ++i) stats[i] = 0;
    stats[0] = P.cnt && ball_enlarged(P);
    stats[1] = P.cnt && P.flat;
    stats[3] = P.cnt;
    stats[9] = GknnNum<T>::max_passes;
    const T inf = static_cast<T>(__builtin_huge_val());
    for (int i = 0; i < n; ++i) {
        for (int o = 0; o < k; ++o) { d2[(size_t)i * k + o] = inf; idx[(size_t)i * k + o] = -1; }
        const T* q = x + (size_t)i * cx;
        if (i >= nb || !(ball_finite(q[0]) && ball_finite(q[1]) && ball_finite(q[2]))) continue;
        const Row<T> p = {q[0], q[1], q[2]};
        T d[K];
        int id[K], sl[K];
        topk_init(d, id, sl, k);
        auto keys = [&](int j) -> uint64_t { return order[j].first; };
        auto row = [&](int j) -> const Row<T>& { return rows4[j]; };
        auto orig = [&](int j) -> int { return order[j].second; };
        const auto ins = topk_inserter(d, id, sl, orig);
        const GknnScan r = gknn_scan<T>(P, d, p, keys, row, ins);
        stats[2] += r.visited;
        stats[4] = std::max<int64_t>(stats[4], r.passes);
        stats[5] += r.growth > 1;
        stats[6] += r.closing > 0;
        stats[7] += r.whole;
        stats[8] += r.passes;
        for (int o = 0; o < k; ++o) { d2[(size_t)i * k + o] = d[K - k + o]; idx[(size_t)i * k + o] = id[K - k + o]; }
    }
}

template <typename T>
void run_k(const T* x, int n, int cx, int nb, const T* y, int m, int cy, int mb, int k, T edge, T* d2, int64_t* idx, int64_t* stats) {
    if (k == 1) run<T, 1>(x, n, cx, nb, y, m, cy, mb, k, edge, d2, idx, stats);
    else if (k <= 8) run<T, 8>(x, n, cx, nb, y, m, cy, mb, k, edge, d2, idx, stats);
    else run<T, 32>(x, n, cx, nb, y, m, cy, mb, k, edge, d2, idx, stats);
}

}  // namespace

extern "C" {

void gk_run_f32(const float* x, int n, int cx, int nb, const float* y, int m, int cy, int mb, int k, float edge, float* d2, int64_t* idx, int64_t* stats) {
    run_k<float>(x, n, cx, nb, y, m, cy, mb, k, edge, d2, idx, stats);
}
void gk_run_f64(const double* x, int n, int cx, int nb, const double* y, int m, int cy, int mb, int k, double edge, double* d2, int64_t* idx, int64_t* stats) {
    run_k<double>(x, n, cx, nb, y, m, cy, mb, k, edge, d2, idx, stats);
}

}
