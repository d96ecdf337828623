// TEST-ONLY host build of dicp_amd/csrc/dicp_ball.h (g++, no GPU): the plan, the cell keys, the range enumeration and the per-query scan
// that the HIP kernels execute, run serially on a grid built on the host, for tests/test_ball_host.py.  Never loaded by dicp_amd.
#include <algorithm>
#include <vector>

#include "../../dicp_amd/csrc/dicp_ball.h"

using namespace dicp;

namespace {

template <typename T> struct Row { T x, y, z; };

// stats: [0..2] the largest span of cells per axis, [3] edge enlarged, [4] flat, [5] candidates in a cell other than the query's,
// [6] rows visited, [7] live rows
template <typename T, int K>
void run(const T* x, int n, int cx, int nb, const T* y, int m, int cy, int mb, T radius, int k, T* d2, int64_t* idx, int32_t* counts, int64_t* stats) {
    T mn[3], mx[3];
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
    const BallPlan<T> P = ball_plan<T>(mn, mx, cnt, radius);
    std::vector<std::pair<uint64_t, int>> order;
    if (P.cnt) for (int j : live) order.push_back({ball_point_key(P, y[(size_t)j * cy], y[(size_t)j * cy + 1], y[(size_t)j * cy + 2]), j});
    std::sort(order.begin(), order.end());
    std::vector<Row<T>> rows4(order.size());
    for (size_t s = 0; s < order.size(); ++s) {
        const T* p = y + (size_t)order[s].second * cy;
        rows4[s] = {p[0], p[1], p[2]};
    }
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    stats[3] = P.cnt && ball_enlarged(P);
    stats[4] = P.cnt && P.flat;
    stats[7] = P.cnt;
    const T inf = static_cast<T>(__builtin_huge_val());
    for (int i = 0; i < n; ++i) {
        for (int o = 0; o < k; ++o) { d2[(size_t)i * k + o] = inf; idx[(size_t)i * k + o] = -1; }
        counts[i] = 0;
        const T* q = x + (size_t)i * cx;
        if (i >= nb || !(ball_finite(q[0]) && ball_finite(q[1]) && ball_finite(q[2]))) continue;
        const Row<T> p = {q[0], q[1], q[2]};
        const uint64_t own = ball_point_key(P, p.x, p.y, p.z);
        T d[K];
        int id[K], sl[K];
        topk_init(d, id, sl, k);
        auto keys = [&](int j) -> uint64_t { return order[j].first; };
        auto row = [&](int j) -> const Row<T>& { return rows4[j]; };
        auto orig = [&](int j) -> int { return order[j].second; };
        const auto put = topk_inserter(d, id, sl, orig);
        auto ins = [&](T v, int j) { if (order[j].first != own) ++stats[5]; put(v, j); };
        const BallScan r = ball_scan<T>(P, p, keys, row, ins);
        counts[i] = r.count;
        stats[6] += r.visited;
        for (int a = 0; a < 3; ++a) stats[a] = std::max<int64_t>(stats[a], r.spans[a]);
        for (int o = 0; o < k; ++o) { d2[(size_t)i * k + o] = d[K - k + o]; idx[(size_t)i * k + o] = id[K - k + o]; }
    }
}

template <typename T>
void run_k(const T* x, int n, int cx, int nb, const T* y, int m, int cy, int mb, T radius, int k, T* d2, int64_t* idx, int32_t* counts, int64_t* stats) {
    if (k == 1) run<T, 1>(x, n, cx, nb, y, m, cy, mb, radius, k, d2, idx, counts, stats);
    else if (k <= 8) run<T, 8>(x, n, cx, nb, y, m, cy, mb, radius, k, d2, idx, counts, stats);
    else run<T, 32>(x, n, cx, nb, y, m, cy, mb, radius, k, d2, idx, counts, stats);
}

}  // namespace

extern "C" {

void bc_run_f32(const float* x, int n, int cx, int nb, const float* y, int m, int cy, int mb, float radius, int k, float* d2, int64_t* idx,
                int32_t* counts, int64_t* stats) {
    run_k<float>(x, n, cx, nb, y, m, cy, mb, radius, k, d2, idx, counts, stats);
}
void bc_run_f64(const double* x, int n, int cx, int nb, const double* y, int m, int cy, int mb, double radius, int k, double* d2, int64_t* idx,
                int32_t* counts, int64_t* stats) {
    run_k<double>(x, n, cx, nb, y, m, cy, mb, radius, k, d2, idx, counts, stats);
}
float bc_R_f32(float r) { return ball_R<float>(r); }
double bc_R_f64(double r) { return ball_R<double>(r); }

}
