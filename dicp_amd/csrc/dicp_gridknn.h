// The exact k-nearest-neighbour scan over the cell grid of dicp_ball.h, without a radius (dicp_amd/knn.py: knn_points / chamfer_distance
// with method="grid"; csrc/knn_grid.hip).
//
// Plain inline C++ templated on the scalar T and on accessors, included by the HIP kernels and by a TEST-ONLY g++ build
// (tests/test_gridknn_host.py) that holds the plan, the keys and the per-query scan to a numpy brute force.
//
// The result is knn_points' own: d2 = topk_d2, the candidates of a query p are the live rows with finite d2, the list is the first
// min(k, #candidates) of them in (d2, original index) order, empty slots hold (+inf, -1).  The list code is dicp_topk.h's: what it holds
// is the k best in that total order of the rows it was fed, whatever order they came in, so ties across cells go to the lowest index
// as long as every row is fed at most once and no row that belongs to the result is left out.
//
// THE PLAN (gknn_plan).  Origin, key widths and the enlarge-until-63-bits loop are ball_plan's; what differs is the starting cell edge,
// one edge s for the three axes, chosen from the cloud's density.  With e_d the extents of the cnt live rows, C = GKNN_ROWS_PER_CELL and
//   cells(s) = prod_d max(e_d / s, 1)                  the cells of the bounding box at edge s, an axis thinner than s counting once
// s is the largest of emax * 2^-i * {1.75, 1.5, 1.25, 1} (emax the largest extent, i <= GKNN_EDGE_HALVINGS) with cells(s) >= cnt / C:
// about C rows per cell for a cloud that fills its box, whether the box is a volume, a wall (one extent zero or below s: that axis
// counts as one cell and the other two share the rows) or a line (two such axes).  A cloud that is a surface inside a volume gets more
// rows per occupied cell (the rule cannot see occupancy); cnt copies of one point (emax = 0) get s = 1 and one cell.  cells(emax) >= 1
// and cells(s) >= emax / s, so the halving ends after at most log2(cnt) + 1 steps.  Every step is an IEEE division, multiplication or
// comparison in double, written one rounding per statement: the host build and the device compute the same edge, bit for bit (no
// cbrt / log2, whose last bit differs between maths libraries).  The edge converted to T must be finite and > 0, or the plan is flat.
// Any s > 0 is correct (the CLAIM of dicp_ball.h holds for any cell edge), only slower.  The plan's R field holds the starting edge,
// so that ball_enlarged tells whether the fit loop changed an edge; r2 is unused (+inf).  At the rule's own edge an axis has at most
// 2^(GKNN_EDGE_HALVINGS + 1) cells and the box about cnt / C, so the fit loop only acts where mx - o overflows T and ends flat; it is
// kept so that the keys fit whatever the rule is (gknn_plan_at takes any edge, and the host tests run it at edges that need the loop).
//
// THE SCAN (gknn_scan) of one query p with three finite coordinates.  It rests on the CLAIM of dicp_ball.h only:
//  (A) for a radius rho (a number of T, > 0) every live row with d2 <= fl(rho * rho) lies in the cell box
//      B(rho) = ball_range_at(P, ball_R(rho), p), the cells cell(fl(p_d - R)) .. cell(fl(p_d + R)) intersected with the grid 0 .. hi_d.
//  (B) The boxes are nested: ball_R is non-decreasing in rho (a rounded product with a constant, the next float up and a maximum all
//      are), fl(p_d - R) is non-increasing and fl(p_d + R) non-decreasing in R, and ball_cell is monotone.  So rho' >= rho gives
//      B(rho') >= B(rho) as sets of cells, and the scan only ever visits the shell B(rho') \ V, V the box visited so far.
//  (C) After all of B(rho) has been fed to the list, a full list whose k-th d2, d_k, is <= fl(rho * rho) is final: every row not yet
//      fed lies outside B(rho), so by (A) its d2 > fl(rho * rho) >= d_k, strictly: it neither enters the list nor ties with its last
//      entry.  (A row with a NaN or +inf d2 is no candidate wherever it lies.)
//  (D) A box that is the whole grid (0 .. hi_d on every axis), or a flat plan (one pass over every live row), ends the scan with
//      whatever the list holds: every live row has been fed.
// Two phases.  GROWTH: rho_0 = the plan's starting edge; pass t feeds the shell B(rho_t) \ B(rho_(t-1)); it ends when the list is full
// or the box is the whole grid; rho_(t+1) = 2 rho_t, or -- when B(rho_t) is empty, the query lying outside the grid -- the larger of
// that and the query's distance to the grid's bounding box on the axis where it is largest (any increasing sequence is correct; this
// one reaches the grid in one step from however far).  CLOSING: with the list full, rho* = the smallest number of T found with
// fl(rho* * rho*) >= d_k -- sqrt(d_k), stepped up while its COMPUTED square is below d_k, BallNum<T>::floor_R for d_k = 0 (ball_R never
// searches less than that); a square that overflows is >= d_k too, and ball_R is then so large that the box is the whole grid.
// If rho* <= the last rho of the growth, (C) holds already; otherwise one more pass feeds B(rho*) \ V.  The list stays full, its k-th
// d2 can only have gone down, so d_k' <= d_k <= fl(rho* * rho*) and (C) ends the scan.
//
// BOUNDS.  Every rho of the growth is at least twice the one before, rho_0 > 0 is a number of T and a rho that overflows to +inf gives
// R = +inf and the whole grid: at most GknnNum<T>::max_passes passes (the doublings between the smallest subnormal and +inf, and the
// closing pass), whatever the coordinates are.  A pass is at most six boxes (the shell cut into slabs), each box ball_scan's column
// jumping enumeration: at most 3 cnt + 2 steps of a log2(cnt) search, and at most cnt rows fed in the whole scan.  An empty
// intersection costs the six divisions of its range and nothing else.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dicp_ball.h"

namespace dicp {

constexpr double GKNN_ROWS_PER_CELL = 2.0;
constexpr int GKNN_EDGE_HALVINGS = 40;                  // cnt <= 2^30 needs 32

template <typename T> struct GknnNum;
template <> struct GknnNum<float>  { static constexpr int max_passes = 149 + 128 + 3; };
template <> struct GknnNum<double> { static constexpr int max_passes = 1074 + 1024 + 3; };

DICP_HD float  gknn_sqrt(float x)  { return sqrtf(x); }
DICP_HD double gknn_sqrt(double x) { return sqrt(x); }

DICP_HD double gknn_cells(const double* e, double s) {
    double c = 1.0;
    for (int d = 0; d < 3; ++d) {
        const double q = e[d] / s;
        const double f = q > 1.0 ? q : 1.0;
        c = c * f;
    }
    return c;
}

// The starting edge of the rule above, in double; 0 where there is none (an extent that is not finite)
DICP_HD double gknn_edge(const double* e, int cnt) {
    double emax = e[0] > e[1] ? e[0] : e[1];
    emax = emax > e[2] ? emax : e[2];
    if (!ball_finite(emax) || !ball_finite(e[0]) || !ball_finite(e[1]) || !ball_finite(e[2])) return 0.0;
    if (!(emax > 0.0)) return 1.0;
    const double target = (double)cnt / GKNN_ROWS_PER_CELL;
    double s = emax;
    for (int i = 0; i < GKNN_EDGE_HALVINGS && gknn_cells(e, s) < target; ++i) s = s * 0.5;
    const double s7 = s * 1.75, s6 = s * 1.5, s5 = s * 1.25;
    if (gknn_cells(e, s7) >= target) return s7;
    if (gknn_cells(e, s6) >= target) return s6;
    if (gknn_cells(e, s5) >= target) return s5;
    return s;
}

// The plan of a cloud at the starting edge s (any s: the scan is exact for every edge > 0, and an edge that is not a finite number > 0
// gives a flat plan).  mn, mx: the per-axis bounds of the cnt live rows of the cloud (unused when cnt = 0)
template <typename T>
DICP_HD BallPlan<T> gknn_plan_at(const T* mn, const T* mx, int cnt, T s) {
    BallPlan<T> P;
    const bool ok = s > T(0) && ball_finite(s);
    P.R = ok ? s : T(1);
    P.r2 = static_cast<T>(__builtin_huge_val());
    P.cnt = cnt > 0 ? cnt : 0;
    P.flat = 1;
    P.wy = P.wz = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) { P.o[d] = P.cnt ? mn[d] : T(0); P.s[d] = P.R; P.hi[d] = 0; }
    if (!P.cnt || !ok) return P;
    int w[3] = {0, 0, 0};
    for (int it = 0; it < BALL_PLAN_STEPS; ++it) {                              // ball_plan's fit: see dicp_ball.h
        bool conv = true;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            int64_t v;
            if (!vox_coord(mx[d], P.o[d], P.s[d], &v) || v < 0) { conv = false; P.s[d] = P.s[d] * T(1073741824); }
            else { P.hi[d] = v; w[d] = vox_width(0, v); }
        }
        if (!(ball_finite(P.s[0]) && ball_finite(P.s[1]) && ball_finite(P.s[2]))) break;
        if (!conv) continue;
        if (w[0] + w[1] + w[2] <= BALL_KEY_BITS) { P.flat = 0; break; }
        if (w[0] >= w[1] && w[0] >= w[2]) P.s[0] = P.s[0] * T(2);
        else if (w[1] >= w[2]) P.s[1] = P.s[1] * T(2);
        else P.s[2] = P.s[2] * T(2);
    }
    if (P.flat) { for (int d = 0; d < 3; ++d) P.hi[d] = 0; return P; }
    P.wy = w[1];
    P.wz = w[2];
    return P;
}

// The plan at the density rule's edge
template <typename T>
DICP_HD BallPlan<T> gknn_plan(const T* mn, const T* mx, int cnt) {
    double e[3] = {0.0, 0.0, 0.0};
    if (cnt > 0) for (int d = 0; d < 3; ++d) e[d] = (double)mx[d] - (double)mn[d];
    return gknn_plan_at<T>(mn, mx, cnt, cnt > 0 ? (T)gknn_edge(e, cnt) : T(0));
}

// The smallest rho found with fl(rho * rho) >= dk, for a finite dk >= 0 (see CLOSING above)
template <typename T>
DICP_HD T gknn_closing_radius(T dk) {
    if (!(dk > T(0))) return BallNum<T>::floor_R;
    T r = gknn_sqrt(dk);
    for (int i = 0; i < 4; ++i) {
        const T q = r * r;
        if (q >= dk) return r;
        r = ball_next_up(r);
    }
    return r * T(2);                                    // (not reached with a correctly rounded sqrt: (2 r)^2 >= dk whatever sqrt did)
}

// The query's distance to the grid's bounding box on the axis where it is largest (0 or less inside; rounded, and only ever a speed-up)
template <typename T>
DICP_HD T gknn_gap(const BallPlan<T>& P, T x, T y, T z) {
    const T p[3] = {x, y, z};
    T g = T(0);
    for (int d = 0; d < 3; ++d) {
        const T n = (T)(P.hi[d] + 1);
        const T w = n * P.s[d];
        const T top = P.o[d] + w;
        const T a = P.o[d] - p[d];
        const T b = p[d] - top;
        if (a > g) g = a;
        if (b > g) g = b;
    }
    return g;
}

// visited: rows fed; passes: boxes computed (growth and closing); growth: those of the growth; closing: rows fed by the closing pass
// (every one of them in a cell outside the growth's box); whole: ended on (D)
struct GknnScan { unsigned visited; int passes; int growth; unsigned closing; int whole; };

// The scan of one query p over a grid: keys(j) / row(j) the sorted key and row of slot j < P.cnt; d the list (K >= k entries, the k-th
// best d2 so far in d[K - 1], +inf until the list is full) that ins(d2, j) feeds.
template <typename T, int K, typename Q, typename Keys, typename Row, typename Ins>
DICP_HD GknnScan gknn_scan(const BallPlan<T>& P, const T (&d)[K], const Q& p, const Keys& keys, const Row& row, const Ins& ins) {
    GknnScan out = {0u, 0, 0, 0u, 0};
    const int cnt = P.cnt;
    if (cnt <= 0) return out;
    auto visit = [&](int j) { ++out.visited; ins(topk_d2<T>(p, row(j)), j); };
    if (P.flat) {
        for (int j = 0; j < cnt; ++j) visit(j);
        out.passes = out.growth = out.whole = 1;
        return out;
    }
    const T inf = static_cast<T>(__builtin_huge_val());
    const uint64_t ymask = vox_shl(1, P.wy) - 1;
    bool have = false;                                  // V = vlo .. vhi, the box visited so far
    int64_t vlo0 = 0, vlo1 = 0, vlo2 = 0, vhi0 = 0, vhi1 = 0, vhi2 = 0;
    bool closing = false;
    T rho = P.R;
    // (one loop for both phases and one for the slabs of a shell, so that the enumeration below is compiled once)
    for (int t = 0; t < GknnNum<T>::max_passes; ++t) {
        ++out.passes;
        if (!closing) ++out.growth;
        const unsigned before = out.visited;
        int64_t lo[3], hi[3];
        bool whole = false;
        if (ball_range_at(P, ball_R(rho), (T)p.x, (T)p.y, (T)p.z, lo, hi)) {       // (empty: V is empty as well, by (B))
            if (have) {                                                             // (B), as a belt
                lo[0] = lo[0] < vlo0 ? lo[0] : vlo0; lo[1] = lo[1] < vlo1 ? lo[1] : vlo1; lo[2] = lo[2] < vlo2 ? lo[2] : vlo2;
                hi[0] = hi[0] > vhi0 ? hi[0] : vhi0; hi[1] = hi[1] > vhi1 ? hi[1] : vhi1; hi[2] = hi[2] > vhi2 ? hi[2] : vhi2;
            }
            // B \ V as at most six disjoint slabs: left and right of V in x; inside V's x range, below and above V in y; inside V's
            // x and y ranges, below and above V in z.  Slab 0 is all of B, for the first box.
            for (int slab = have ? 1 : 0; slab < (have ? 7 : 1); ++slab) {
                int64_t x0 = lo[0], x1 = hi[0], y0 = lo[1], y1 = hi[1], z0 = lo[2], z1 = hi[2];
                if (slab == 1) x1 = vlo0 - 1;
                else if (slab == 2) x0 = vhi0 + 1;
                else if (slab >= 3) {
                    x0 = vlo0; x1 = vhi0;
                    if (slab == 3) y1 = vlo1 - 1;
                    else if (slab == 4) y0 = vhi1 + 1;
                    else {
                        y0 = vlo1; y1 = vhi1;
                        if (slab == 5) z1 = vlo2 - 1; else z0 = vhi2 + 1;
                    }
                }
                if (x0 > x1 || y0 > y1 || z0 > z1) continue;
                // the rows of the cells x0 .. x1, y0 .. y1, z0 .. z1: ball_scan's enumeration (dicp_ball.h) -- a column (cx, cy) is one
                // contiguous range of slots, a column without rows is skipped to the next one that has any
                int64_t cx = x0, cy = y0;
                while (cx <= x1) {
                    const uint64_t k_lo = ball_key(P, cx, cy, z0), k_hi = ball_key(P, cx, cy, z1);
                    int j = ball_lower_bound(keys, cnt, k_lo);
                    if (j >= cnt) break;
                    const uint64_t kj = keys(j);
                    if (kj <= k_hi) {
                        do { visit(j); ++j; } while (j < cnt && keys(j) <= k_hi);
                    } else {
                        const uint64_t col = kj >> P.wz;
                        const int64_t kx = (int64_t)(col >> P.wy), ky = (int64_t)(col & ymask);
                        if (kx > cx || ky > cy) {
                            const int64_t ty = kx > cx ? (ky < y0 ? y0 : ky) : ky;
                            cx = kx;
                            if (ty > y1) { ++cx; cy = y0; } else cy = ty;
                            continue;
                        }
                    }
                    if (++cy > y1) { ++cx; cy = y0; }
                }
            }
            have = true;
            vlo0 = lo[0]; vlo1 = lo[1]; vlo2 = lo[2]; vhi0 = hi[0]; vhi1 = hi[1]; vhi2 = hi[2];
            whole = lo[0] == 0 && lo[1] == 0 && lo[2] == 0 && hi[0] == P.hi[0] && hi[1] == P.hi[1] && hi[2] == P.hi[2];
        }
        if (closing) out.closing = out.visited - before;
        if (whole) { out.whole = 1; break; }            // (D)
        if (closing) break;                             // (C) at rho*
        if (d[K - 1] < inf) {                           // the list is full: the growth is over
            const T star = gknn_closing_radius(d[K - 1]);
            if (star <= rho) break;                     // (C) at the growth's last rho
            rho = star;
            closing = true;
            continue;
        }
        T next = rho * T(2);
        if (!have) {
            const T g = gknn_gap(P, (T)p.x, (T)p.y, (T)p.z);
            if (g > next) next = g;
        }
        rho = next;
    }
    return out;
}

}  // namespace dicp
