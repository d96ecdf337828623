// TEST-ONLY host build of dicp_amd/csrc/dicp_iss_ball.h (g++, no GPU): the whole-ball member walk and the two passes that the HIP kernels
// of csrc/iss_ball.hip execute, run serially on a grid built and sorted on the host, for tests/test_iss_ball_host.py.  Never loaded by
// dicp_amd.
//
// variant 0 is the header's rule.  variant 1 is a WRONG rule, written out here, which the comparison with tests/iss_ball_ref.py must
// refuse: the members are taken in ROW order instead of grid order (same members, same counts, other sums).
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../dicp_amd/csrc/dicp_iss_ball.h"

using namespace dicp;

namespace {

enum { RIGHT = 0, ROW_ORDER = 1 };

template <typename T> struct Row { T x, y, z; };

template <typename T>
struct Grid {
    BallPlan<T> P;
    std::vector<std::pair<uint64_t, int>> order;            // (key, row) of the live rows, sorted
    std::vector<Row<T>> rows4;
    std::vector<int> slot_of;                               // row -> sorted slot, -1 for a row outside the grid
};

// the grid dicp_ball_grid_build makes of one cloud at the radius `rT` of T
template <typename T>
Grid<T> build(const T* pts, int c, int m, int rows, T rT) {
    Grid<T> G;
    T mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    int cnt = 0;
    std::vector<int> live;
    for (int j = 0; j < std::min(std::max(rows, 0), m); ++j) {
        const T* p = pts + (size_t)j * c;
        if (!(ball_finite(p[0]) && ball_finite(p[1]) && ball_finite(p[2]))) continue;
        for (int d = 0; d < 3; ++d) {
            mn[d] = cnt ? std::min(mn[d], p[d]) : p[d];
            mx[d] = cnt ? std::max(mx[d], p[d]) : p[d];
        }
        ++cnt;
        live.push_back(j);
    }
    G.P = ball_plan<T>(mn, mx, cnt, rT);
    if (G.P.cnt) for (int j : live) G.order.push_back({ball_point_key(G.P, pts[(size_t)j * c], pts[(size_t)j * c + 1], pts[(size_t)j * c + 2]), j});
    std::sort(G.order.begin(), G.order.end());
    G.rows4.resize(G.order.size());
    G.slot_of.assign((size_t)m, -1);
    for (size_t s = 0; s < G.order.size(); ++s) {
        const T* p = pts + (size_t)G.order[s].second * c;
        G.rows4[s] = {p[0], p[1], p[2]};
        G.slot_of[(size_t)G.order[s].second] = (int)s;
    }
    return G;
}

// variant 1: pass 1 of row i with the members in row order
template <typename T>
double saliency_row_order(const T* pts, int c, const Grid<T>& G, int i, double radius2, double g21, double g32, int min_nb, double* l, int& count) {
    double pi[3] = {(double)pts[(size_t)i * c], (double)pts[(size_t)i * c + 1], (double)pts[(size_t)i * c + 2]};
    double sum[3] = {0.0, 0.0, 0.0};
    int n = 1;
    const int m = (int)G.slot_of.size();
    for (int walk = 0; walk < 2; ++walk) {
        double mu[3], a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const double zero[3] = {0.0, 0.0, 0.0};
        if (walk) { iss_mean(sum, n, mu); iss_cov_add(a, zero, mu); }
        for (int j = 0; j < m; ++j) {
            if (j == i || G.slot_of[(size_t)j] < 0) continue;
            double pj[3] = {(double)pts[(size_t)j * c], (double)pts[(size_t)j * c + 1], (double)pts[(size_t)j * c + 2]}, q[3];
            if (!iss_member(true, iss_d2(pi, pj, q), radius2)) continue;
            if (walk) iss_cov_add(a, q, mu); else { ++n; iss_mean_add(sum, q); }
        }
        if (walk) {
            iss_cov_scale(a, n);
            iss_eigenvalues(a, l);
        }
    }
    count = n;
    return iss_saliency(l, n, g21, g32, min_nb);
}

// both passes of one cloud; stats: [0] rows visited by pass 1, [1] by pass 2, [2] edge enlarged, [3] flat, [4] live rows
template <typename T>
void cloud(const T* pts, int c, int m, int rows, double r1, double r2, double g21, double g32, int min_nb, int variant, T* eig, T* sal_out,
           int32_t* cnt, uint8_t* mask, int64_t* order_out, int64_t* stats) {
    const Grid<T> G = build<T>(pts, c, m, rows, iss_ball_grid_radius<T>(r1 > r2 ? r1 : r2));
    for (int i = 0; i < 5; ++i) stats[i] = 0;
    stats[2] = G.P.cnt && ball_enlarged(G.P);
    stats[3] = G.P.cnt && G.P.flat;
    stats[4] = G.P.cnt;
    for (int i = 0; i < m; ++i) order_out[i] = i < (int)G.order.size() ? G.order[(size_t)i].second : -1;
    auto keys = [&](int j) -> uint64_t { return G.order[(size_t)j].first; };
    auto row = [&](int j) -> const Row<T>& { return G.rows4[(size_t)j]; };
    auto orig = [&](int j) -> int { return G.order[(size_t)j].second; };
    std::vector<double> sal((size_t)m, 0.0);
    for (int i = 0; i < m; ++i) {
        double l[3] = {0.0, 0.0, 0.0};
        int count = 0;
        const int s = G.slot_of[(size_t)i];
        if (s >= 0) {
            unsigned visited = 0;
            if (variant == ROW_ORDER) sal[(size_t)i] = saliency_row_order<T>(pts, c, G, i, r1 * r1, g21, g32, min_nb, l, count);
            else sal[(size_t)i] = iss_ball_saliency_row<T>(G.P, iss_ball_R<T>(r1), r1 * r1, s, keys, row, g21, g32, min_nb, l, count, visited);
            stats[0] += visited;
        }
        sal_out[i] = (T)sal[(size_t)i];
        for (int a = 0; a < 3; ++a) eig[(size_t)i * 3 + a] = (T)l[a];
        cnt[i] = count;
    }
    auto salj = [&](int j) -> double { return sal[(size_t)orig(j)]; };
    for (int i = 0; i < m; ++i) {
        const int s = G.slot_of[(size_t)i];
        bool keep = false;
        if (s >= 0 && sal[(size_t)i] > 0.0) {
            unsigned visited = 0;
            keep = iss_ball_maximum_row<T>(G.P, iss_ball_R<T>(r2), r2 * r2, s, i, sal[(size_t)i], min_nb, keys, row, salj, orig, visited);
            stats[1] += visited;
        }
        mask[i] = keep ? 1 : 0;
    }
}

// The coverage claim alone: mem (m, m) bytes, mem[i, j] = 1 when the walk of row i at `radius` on the grid built at `grid_radius` VISITS
// row j != i and iss_member accepts it.  stats: [0] rows visited, [1] the largest span of cells on an axis, [2] enlarged, [3] flat,
// [4] visits of a row already visited by the same walk (must stay 0), [5] members in a cell other than the row's own
template <typename T>
void members(const T* pts, int c, int m, int rows, double grid_radius, double radius, uint8_t* mem, int64_t* stats) {
    const Grid<T> G = build<T>(pts, c, m, rows, iss_ball_grid_radius<T>(grid_radius));
    for (int i = 0; i < 6; ++i) stats[i] = 0;
    stats[2] = G.P.cnt && ball_enlarged(G.P);
    stats[3] = G.P.cnt && G.P.flat;
    auto keys = [&](int j) -> uint64_t { return G.order[(size_t)j].first; };
    const T R = iss_ball_R<T>(radius);
    const double radius2 = radius * radius;
    std::vector<uint8_t> seen;
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < m; ++j) mem[(size_t)i * m + j] = 0;
        const int s = G.slot_of[(size_t)i];
        if (s < 0) continue;
        const Row<T>& p = G.rows4[(size_t)s];
        double pi[3];
        iss_ball_load(p, pi);
        int64_t lo[3], hi[3];
        if (!G.P.flat && ball_range_at(G.P, R, p.x, p.y, p.z, lo, hi))
            for (int d = 0; d < 3; ++d) stats[1] = std::max<int64_t>(stats[1], hi[d] - lo[d] + 1);
        seen.assign(G.order.size(), 0);
        stats[0] += iss_ball_scan<T>(G.P, R, p.x, p.y, p.z, keys, [&](int j) {
            if (seen[(size_t)j]) ++stats[4];
            seen[(size_t)j] = 1;
            if (j == s) return false;
            double pj[3], q[3];
            iss_ball_load(G.rows4[(size_t)j], pj);
            if (iss_member(true, iss_d2(pi, pj, q), radius2)) {
                mem[(size_t)i * m + G.order[(size_t)j].second] = 1;
                if (G.order[(size_t)j].first != G.order[(size_t)s].first) ++stats[5];
            }
            return false;
        });
    }
}

// the plan of one cloud at the grid radius of `radius`: edges (3) as doubles, flags: enlarged, flat, live rows
template <typename T>
void plan(const T* pts, int c, int m, int rows, double radius, double* edges, int32_t* flags) {
    const Grid<T> G = build<T>(pts, c, m, rows, iss_ball_grid_radius<T>(radius));
    for (int d = 0; d < 3; ++d) edges[d] = (double)G.P.s[d];
    flags[0] = G.P.cnt && ball_enlarged(G.P);
    flags[1] = G.P.cnt && G.P.flat;
    flags[2] = G.P.cnt;
}

}  // namespace

extern "C" {

void ibc_cloud(int f64, const void* pts, int c, int m, int rows, double r1, double r2, double g21, double g32, int min_nb, int variant, void* eig,
               void* sal, int32_t* cnt, uint8_t* mask, int64_t* order, int64_t* stats) {
    if (f64) cloud<double>((const double*)pts, c, m, rows, r1, r2, g21, g32, min_nb, variant, (double*)eig, (double*)sal, cnt, mask, order, stats);
    else cloud<float>((const float*)pts, c, m, rows, r1, r2, g21, g32, min_nb, variant, (float*)eig, (float*)sal, cnt, mask, order, stats);
}
void ibc_members(int f64, const void* pts, int c, int m, int rows, double grid_radius, double radius, uint8_t* mem, int64_t* stats) {
    if (f64) members<double>((const double*)pts, c, m, rows, grid_radius, radius, mem, stats);
    else members<float>((const float*)pts, c, m, rows, grid_radius, radius, mem, stats);
}
void ibc_plan(int f64, const void* pts, int c, int m, int rows, double radius, double* edges, int32_t* flags) {
    if (f64) plan<double>((const double*)pts, c, m, rows, radius, edges, flags);
    else plan<float>((const float*)pts, c, m, rows, radius, edges, flags);
}
// the grid radius and the half-width of a pass in T, as doubles
void ibc_radii(int f64, double r, double* out) {
    if (f64) { out[0] = iss_ball_grid_radius<double>(r); out[1] = iss_ball_R<double>(r); }
    else { out[0] = (double)iss_ball_grid_radius<float>(r); out[1] = (double)iss_ball_R<float>(r); }
}

}
