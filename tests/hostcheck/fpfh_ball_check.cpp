// TEST-ONLY host build of dicp_amd/csrc/dicp_fpfh_ball.h (g++, no GPU): the whole-ball near list and the two passes that the HIP kernels
// of csrc/fpfh_ball.hip execute, run serially on a grid built and sorted on the host, for tests/test_fpfh_ball_host.py.  Never loaded by
// dicp_amd.
//
// variant 0 is the header's rule.  variant 1 is a WRONG rule, written out here, which the comparison with tests/fpfh_ball_ref.py must
// refuse: the near list is taken in ROW order instead of grid order (same rows, same counts, another order of the weighted sum).
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../dicp_amd/csrc/dicp_fpfh_ball.h"

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

// One cloud: the pack, pass 1 on every slot, pass 2 on every row (at == nullptr: out (m, 33)) or on the q entries of at (out (q, 33)).
// spfh (m, 33) int32; order_out (m) the sorted rows, -1 behind them; stats: [0] rows visited by pass 1, [1] by pass 2, [2] edge enlarged,
// [3] flat, [4] live rows
template <typename T, typename I>
void cloud(const T* pts, int c, const T* nrm, int m, int rows, double radius, int variant, const I* at, int q, T* out, int32_t* spfh,
           int64_t* order_out, int64_t* stats) {
    const Grid<T> G = build<T>(pts, c, m, rows, iss_ball_grid_radius<T>(radius));
    const int cnt = (int)G.order.size();
    for (int i = 0; i < 5; ++i) stats[i] = 0;
    stats[2] = G.P.cnt && ball_enlarged(G.P);
    stats[3] = G.P.cnt && G.P.flat;
    stats[4] = G.P.cnt;
    for (int i = 0; i < m; ++i) order_out[i] = i < cnt ? G.order[(size_t)i].second : -1;
    const T R = iss_ball_R<T>(radius);
    const double radius2 = radius * radius;
    auto keys = [&](int j) -> uint64_t { return G.order[(size_t)j].first; };
    auto row = [&](int j) -> const Row<T>& { return G.rows4[(size_t)j]; };
    // the pack: the normals and the OK flags in slot order
    std::vector<double> n3((size_t)cnt * 3);
    std::vector<uint8_t> okf((size_t)cnt);
    for (int s = 0; s < cnt; ++s) {
        const int i = G.order[(size_t)s].second;
        double p[3];
        iss_ball_load(G.rows4[(size_t)s], p);
        for (int a = 0; a < 3; ++a) n3[(size_t)s * 3 + a] = (double)nrm[(size_t)i * 3 + a];
        okf[(size_t)s] = fpfh_row_ok(p, &n3[(size_t)s * 3]);
    }
    auto nrm_of = [&](int j, double* n) -> bool {
        for (int a = 0; a < 3; ++a) n[a] = n3[(size_t)j * 3 + a];
        return okf[(size_t)j] != 0;
    };
    // the near list of slot s in ROW order (variant 1): the slots sorted by their row index
    std::vector<int> by_row((size_t)cnt);
    for (int s = 0; s < cnt; ++s) by_row[(size_t)s] = s;
    std::sort(by_row.begin(), by_row.end(), [&](int a, int b) { return G.order[(size_t)a].second < G.order[(size_t)b].second; });
    auto near_row_order = [&](int s, auto ok, auto near) {
        double pi[3];
        iss_ball_load(G.rows4[(size_t)s], pi);
        for (int j : by_row) {
            if (j == s) continue;
            double pj[3], d[3];
            iss_ball_load(G.rows4[(size_t)j], pj);
            const double r2 = fpfh_d2(pi, pj, d);
            if (fpfh_near(true, true, r2, radius2) && fpfh_near(true, ok(j), r2, radius2)) near(j, r2, d);
        }
    };
    // pass 1
    std::vector<double> table((size_t)cnt * FPFH_BALL_ROW);
    for (int i = 0; i < m * FPFH_CH; ++i) spfh[i] = 0;
    for (int s = 0; s < cnt; ++s) {
        int counts[FPFH_CH] = {0};
        if (okf[(size_t)s]) {
            const double* ni = &n3[(size_t)s * 3];
            auto add = [&](const int* ch) { ++counts[ch[0]]; ++counts[ch[1]]; ++counts[ch[2]]; };
            if (variant == ROW_ORDER) {
                double nj[3];
                near_row_order(s, [&](int j) { return nrm_of(j, nj); }, [&](int, double r2, double* d) {
                    int ch[3];
                    if (fpfh_pair_bins(ni, nj, d, r2, ch)) add(ch);
                });
            } else {
                stats[0] += fpfh_ball_spfh_row<T>(G.P, R, radius2, s, ni, keys, row, nrm_of, add);
            }
        }
        fpfh_ball_table_row([&](int ch) { return counts[ch]; }, okf[(size_t)s] != 0, &table[(size_t)s * FPFH_BALL_ROW]);
        for (int ch = 0; ch < FPFH_CH; ++ch) spfh[(size_t)G.order[(size_t)s].second * FPFH_CH + ch] = counts[ch];
    }
    // pass 2
    auto tab = [&](int j) -> const double* { return &table[(size_t)j * FPFH_BALL_ROW]; };
    auto inv = [&](int i) -> int { return G.slot_of[(size_t)i]; };
    const int entries = at ? q : m;
    for (int e = 0; e < entries; ++e) {
        int s = at ? fpfh_ball_at(at[e], m, inv) : G.slot_of[(size_t)e];
        T* o = out + (size_t)e * FPFH_CH;
        for (int ch = 0; ch < FPFH_CH; ++ch) o[ch] = T(0);
        if (s < 0 || !okf[(size_t)s]) continue;
        double acc[FPFH_CH];
        if (variant == ROW_ORDER) {
            for (int ch = 0; ch < FPFH_CH; ++ch) acc[ch] = 0.0;
            const double* tj = nullptr;
            near_row_order(s, [&](int j) { tj = tab(j); return tj[FPFH_CH] != 0.0; }, [&](int, double r2, double*) {
                const double wt = fpfh_weight(r2);
                for (int ch = 0; ch < FPFH_CH; ++ch) acc[ch] = fpfh_weight_add(acc[ch], wt, tj[ch]);
            });
        } else {
            stats[1] += fpfh_ball_combine_row<T>(G.P, R, radius2, s, keys, row, tab, acc);
        }
        fpfh_ball_out(acc, tab(s), [&](int ch, double v) { o[ch] = (T)v; });
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

template <typename T>
void cloud_at(const T* pts, int c, const T* nrm, int m, int rows, double radius, int variant, const void* at, int at64, int q, T* out, int32_t* spfh,
              int64_t* order, int64_t* stats) {
    if (at && at64) cloud<T, int64_t>(pts, c, nrm, m, rows, radius, variant, (const int64_t*)at, q, out, spfh, order, stats);
    else cloud<T, int32_t>(pts, c, nrm, m, rows, radius, variant, (const int32_t*)at, q, out, spfh, order, stats);
}

}  // namespace

extern "C" {

void fbc_cloud(int f64, const void* pts, int c, const void* nrm, int m, int rows, double radius, int variant, const void* at, int at64, int q,
               void* out, int32_t* spfh, int64_t* order, int64_t* stats) {
    if (f64) cloud_at<double>((const double*)pts, c, (const double*)nrm, m, rows, radius, variant, at, at64, q, (double*)out, spfh, order, stats);
    else cloud_at<float>((const float*)pts, c, (const float*)nrm, m, rows, radius, variant, at, at64, q, (float*)out, spfh, order, stats);
}
void fbc_plan(int f64, const void* pts, int c, int m, int rows, double radius, double* edges, int32_t* flags) {
    if (f64) plan<double>((const double*)pts, c, m, rows, radius, edges, flags);
    else plan<float>((const float*)pts, c, m, rows, radius, edges, flags);
}

}
