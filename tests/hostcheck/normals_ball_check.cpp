// TEST-ONLY host build of dicp_amd/csrc/dicp_normals_ball.h (g++, no GPU): the forward, the records and the gather that the HIP kernels of
// csrc/normals_ball.hip execute, run serially on a grid built and sorted on the host, for tests/test_normals_ball_host.py.  Never loaded
// by dicp_amd.
//
// variant 0 is the header's rule.  variant 1 is a WRONG rule, written out here, which the comparison with tests/normals_ball_ref.py must
// refuse: the gather sums the members in ROW order instead of grid order (same members, other sums).
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../dicp_amd/csrc/dicp_normals_ball.h"

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

// the grid dicp_ball_grid_build makes of one cloud at the radius `rT` of T (as tests/hostcheck/iss_ball_check.cpp)
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

// the forward of one cloud; state (m, NBL_STATE) BY ORIGINAL ROW (zeros for rows outside the grid); stats: [0] rows visited, [1] enlarged,
// [2] flat, [3] live rows
template <typename T>
void forward(const T* pts, int c, int m, int rows, double radius, const double* vp, int min_nb, T* nrm, T* curv, T* eig, int32_t* cnt,
             int64_t* order_out, double* state, int64_t* stats) {
    const Grid<T> G = build<T>(pts, c, m, rows, iss_ball_grid_radius<T>(radius));
    stats[0] = 0;
    stats[1] = G.P.cnt && ball_enlarged(G.P);
    stats[2] = G.P.cnt && G.P.flat;
    stats[3] = G.P.cnt;
    for (int i = 0; i < m; ++i) order_out[i] = i < (int)G.order.size() ? G.order[(size_t)i].second : -1;
    auto keys = [&](int j) -> uint64_t { return G.order[(size_t)j].first; };
    auto row = [&](int j) -> const Row<T>& { return G.rows4[(size_t)j]; };
    const double origin[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < m; ++i) {
        double l[3] = {0.0, 0.0, 0.0}, n3[3] = {0.0, 0.0, 0.0}, k = 0.0, st[NBL_STATE];
        for (int e = 0; e < NBL_STATE; ++e) st[e] = 0.0;
        int count = 0;
        const int s = G.slot_of[(size_t)i];
        if (s >= 0) {
            unsigned visited = 0;
            nbl_forward_row<T>(G.P, iss_ball_R<T>(radius), radius * radius, s, keys, row, vp ? vp : origin, min_nb, l, n3, k, st, count, visited);
            stats[0] += visited;
        }
        for (int a = 0; a < 3; ++a) { nrm[(size_t)i * 3 + a] = (T)n3[a]; eig[(size_t)i * 3 + a] = (T)l[a]; }
        curv[i] = (T)k;
        cnt[i] = count;
        for (int e = 0; e < NBL_STATE; ++e) state[(size_t)i * NBL_STATE + e] = st[e];
    }
}

// records (m, 13) BY ORIGINAL ROW from the state forward() left and the cotangents gn (m, 3) / gk (m) of T, either may be null
template <typename T>
void records(const T* pts, int c, int m, const double* state, const uint8_t* live, const T* gn, const T* gk, double* rec) {
    for (int i = 0; i < m; ++i) {
        double p[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0}, k = 0.0;
        if (live[i]) {
            for (int a = 0; a < 3; ++a) p[a] = (double)pts[(size_t)i * c + a];
            if (gn) for (int a = 0; a < 3; ++a) g[a] = (double)gn[(size_t)i * 3 + a];
            if (gk) k = (double)gk[i];
        }
        nbl_record(live[i] != 0, state + (size_t)i * NBL_STATE, p, gn != nullptr, g, gk != nullptr, k, sizeof(T) == 4 ? 1e-6 : 1e-12,
                   rec + (size_t)i * NRM_REC);
    }
}

// the gather of one cloud from records BY ORIGINAL ROW; stats: [0] rows visited
template <typename T>
void gather(const T* pts, int c, int m, int rows, double radius, const double* rec, int variant, T* grad, int64_t* stats) {
    const Grid<T> G = build<T>(pts, c, m, rows, iss_ball_grid_radius<T>(radius));
    stats[0] = 0;
    auto keys = [&](int j) -> uint64_t { return G.order[(size_t)j].first; };
    auto row = [&](int j) -> const Row<T>& { return G.rows4[(size_t)j]; };
    auto recs = [&](int j) -> const double* { return rec + (size_t)G.order[(size_t)j].second * NRM_REC; };
    for (int j = 0; j < m; ++j) {
        double g[3] = {0.0, 0.0, 0.0};
        const int s = G.slot_of[(size_t)j];
        if (s >= 0 && variant == RIGHT) {
            unsigned visited = 0;
            nbl_gather_row<T>(G.P, iss_ball_R<T>(radius), radius * radius, s, keys, row, recs, g, visited);
            stats[0] += visited;
        } else if (s >= 0) {
            double pj[3];
            iss_ball_load(G.rows4[(size_t)s], pj);
            nbl_gather_add(rec + (size_t)j * NRM_REC, pj, g);
            for (int i = 0; i < m; ++i) {
                if (i == j || G.slot_of[(size_t)i] < 0) continue;
                double pi[3], q[3];
                iss_ball_load(G.rows4[(size_t)G.slot_of[(size_t)i]], pi);
                if (iss_member(true, iss_d2(pj, pi, q), radius * radius)) nbl_gather_add(rec + (size_t)i * NRM_REC, pj, g);
            }
        }
        for (int a = 0; a < 3; ++a) grad[(size_t)j * 3 + a] = (T)g[a];
    }
}

}  // namespace

extern "C" {

void nbc_forward(int f64, const void* pts, int c, int m, int rows, double radius, const double* vp, int min_nb, void* nrm, void* curv, void* eig,
                 int32_t* cnt, int64_t* order, double* state, int64_t* stats) {
    if (f64) forward<double>((const double*)pts, c, m, rows, radius, vp, min_nb, (double*)nrm, (double*)curv, (double*)eig, cnt, order, state, stats);
    else forward<float>((const float*)pts, c, m, rows, radius, vp, min_nb, (float*)nrm, (float*)curv, (float*)eig, cnt, order, state, stats);
}
void nbc_records(int f64, const void* pts, int c, int m, const double* state, const uint8_t* live, const void* gn, const void* gk, double* rec) {
    if (f64) records<double>((const double*)pts, c, m, state, live, (const double*)gn, (const double*)gk, rec);
    else records<float>((const float*)pts, c, m, state, live, (const float*)gn, (const float*)gk, rec);
}
void nbc_gather(int f64, const void* pts, int c, int m, int rows, double radius, const double* rec, int variant, void* grad, int64_t* stats) {
    if (f64) gather<double>((const double*)pts, c, m, rows, radius, rec, variant, (double*)grad, stats);
    else gather<float>((const float*)pts, c, m, rows, radius, rec, variant, (float*)grad, stats);
}
// n matrices a (n, 6): lam (n, 3), v (n, 9: three rows of 3) of nbl_eigen and iss_lam (n, 3) of iss_eigenvalues
void nbc_eigen(int n, const double* a, double* lam, double* v, double* iss_lam) {
    for (int i = 0; i < n; ++i) {
        double x[6], y[6];
        for (int e = 0; e < 6; ++e) x[e] = y[e] = a[(size_t)i * 6 + e];
        nbl_eigen(x, lam + (size_t)i * 3, v + (size_t)i * 9);
        iss_eigenvalues(y, iss_lam + (size_t)i * 3);
    }
}
// nbl_sign of n pairs (v0, d)
void nbc_sign(int n, const double* v0, const double* d, double* s) {
    for (int i = 0; i < n; ++i) s[i] = nbl_sign(v0 + (size_t)i * 3, d + (size_t)i * 3);
}

}
