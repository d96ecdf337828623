// The whole-ball member list of the ISS keypoint detector (dicp_amd/iss.py: iss_saliency_ball / iss_keypoints_ball; csrc/iss_ball.hip):
// every row of the ball, found by walking the cloud's cell grid (csrc/dicp_ball.h), instead of the k <= 32 slots of a neighbour index.
//
// Plain inline C++ templated on the scalar T of the points and on accessors, included by the HIP kernels and by a TEST-ONLY g++ build
// (tests/test_iss_ball_host.py) that holds the scan and the two passes to numpy (tests/iss_ball_ref.py) on a CPU box with no GPU.
//
// DEFINITION.  Everything of csrc/dicp_iss.h stands and is used unchanged -- iss_row_ok, iss_d2, iss_member, iss_mean_add, iss_mean,
// iss_cov_add, iss_cov_scale, iss_eigenvalues, iss_saliency, iss_beats --; only the member list changes.
//   LIVE rows of a cloud: j < rows[b] with three finite coordinates (OK rows: exactly the rows the cloud's cell grid holds).
//   MEMBERS of a live row i for a radius R (a double, radius2 = fl(R R) in double): row i itself first, then every OTHER live row j with
//     iss_d2(p_i, p_j) <= radius2 -- the double rule of iss_member: the three products rounded, (xx + yy) + zz, inclusive, duplicates at
//     distance 0 included -- in ASCENDING (cell key, row index) ORDER.  That is the order of the sorted slots of the cloud's grid
//     (dicp_ball_grid_build: a bitonic sort of distinct (key, row index) pairs, hence a total order that no network changes).  A row is a
//     member once, whatever the layout; count includes the row itself.
//   The grid of a call is built on the points' dtype T at ONE radius: iss_ball_grid_radius<T>(max(salient, non-max radius)), the smallest
//     T that is not below the double radius (a float32 conversion can round DOWN: then the next float up), or the largest finite T where
//     that would be infinite.  The cell key of a row is dicp_ball.h's: cell_d(a) = floor(fl(fl(a - o_d) / s_d)) in T with o the per-axis
//     minimum of the live rows and s_d = ball_R(grid radius) unless the plan enlarged an edge; a flat grid has every key 0 and the order
//     is the row order.
//   Saliency (pass 1), two walks exactly as iss_saliency_kernel walks its slots twice: walk 1 sums q = p_j - p_i over the members from +0
//     and counts them; mu = sum / count; walk 2 adds d = q - mu of the row itself (q = 0) and then of the members, in the same order, to
//     the six sums; then iss_cov_scale, iss_eigenvalues, iss_saliency.  NOT raw second moments: that is another arithmetic.
//   Maxima (pass 2): dicp_iss.h's rule over the members at the non-max radius on the double saliencies; the order does not matter there.
//     The walk stops at the first member that beats the row: mask = (no member beats it) and count >= min_neighbors, so once a member
//     beats the row the count is not needed any more.
//
// COVERAGE CLAIM.  Let r be a finite double radius > 0, rT = iss_ball_grid_radius<T>(r) and R = ball_R<T>(rT) (iss_ball_R<T>(r)).  If R
// is finite, every live row y with iss_d2(p, y) <= fl(r r) (the DOUBLE rule) has, on every axis d and for every cell edge s_d > 0,
//   cell_d(fl(p_d - R)) <= cell_d(y_d) <= cell_d(fl(p_d + R))          with fl the rounding of T and p, y numbers of T.
// So iss_ball_scan visits EVERY row of those cells (intersected with the grid's cells 0 .. hi_d, which hold all live rows) and the
// caller applies iss_member to each: the scan has no distance filter of its own.  ball_scan's filter, topk_d2<T> <= P.r2 in T, is another
// predicate (in float32 it rounds the differences and products to 24 bits and can differ from the double rule at the border either
// way), so ball_scan itself is not used.
// PROOF.  u64 = 2^-53, eta64 = 2^-1074; uT, etaT those of T (uT >= u64).
//  (a) The inputs of iss_d2 are the exactly converted points; e = fl64(y_d - p_d) and xx = fl64(e e) are dicp_ball.h's steps (1)-(3) with
//      T = double: a member has xx <= fl64(r r), hence in exact reals |y_d - p_d| <= r (1 + 5 u64) if r >= b / u64 (b = 1.01 sqrt(eta64)),
//      and |y_d - p_d| < 1.2 sqrt(eta64) / u64 <= 2^-483 otherwise (steps (2)-(4) there, verbatim).
//  (b) R >= r (1 + 5 u64) in the first case and R >= 2^-483 always.  ball_R<T>(rT) = max(next_up(fl(rT (1 + 8 uT))), floor_R<T>) with
//      floor_R = 2^-49 / 2^-483 >= 2^-483.
//      T = double: rT = r and this is dicp_ball.h's own step (4): r >= b / u64 makes the product normal and R >= r (1 + 6 u64).
//      T = float: fl(rT (1 + 8 uT)) >= rT (rT is a float not above the exact product and rounding is monotone), so R >= next_up(rT); and
//      next_up(x) >= x (1 + 5 u64) for every float x > 0: for a normal x in [2^e, 2^(e+1)) the gap to the next float is 2^(e-23) >
//      x 2^-24 > 5 x 2^-53, for a subnormal x (x < 2^-126) the gap 2^-149 exceeds 5 x 2^-53.  With rT >= r (rT not clamped):
//      R >= rT (1 + 5 u64) >= r (1 + 5 u64).  Where rT was clamped to FLT_MAX (r beyond float's range), fl(rT (1 + 8 uT)) overflows,
//      R = +inf and the claim is not needed: ball_plan makes a grid with an infinite R flat, a pass with an infinite half-width has
//      the whole grid as its range (ball_cell saturates), and either way every live row is visited.
//  (c) So p_d - R <= y_d <= p_d + R in exact reals; y_d is a number of T and rounding to T is monotone: fl(p_d - R) <= y_d <= fl(p_d + R).
//  (d) cell_d is non-decreasing (dicp_ball.h (6)), for ANY s_d > 0: the grid may have been built at a radius other than r (pass 2 walks
//      the grid of the larger radius with the half-width of its own), only the number of rows visited changes.  QED.
// The scan below is ball_scan's loop with `visit every row of the range` in place of the filter: the same enumeration (ball_range_at at
// the pass's half-width, ball_key, ball_lower_bound, the jump over empty columns, the flat case) and the same bound: at most
// 3 cnt + 2 passes of the outer loop, each a binary search, and at most cnt rows visited -- bounded by the cloud's row count whatever
// the coordinates are.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "dicp_ball.h"
#include "dicp_iss.h"

namespace dicp {

// the smallest T >= r, the largest finite T where that is infinite (r finite and > 0)
template <typename T> DICP_HD T iss_ball_grid_radius(double r);
template <> DICP_HD double iss_ball_grid_radius<double>(double r) { return r; }
template <> DICP_HD float iss_ball_grid_radius<float>(double r) {
    if (r >= (double)FLT_MAX) return FLT_MAX;
    const float f = (float)r;
    return (double)f < r ? ball_next_up(f) : f;             // (next_up of a float below FLT_MAX is finite)
}
// the half-width of the cell range of a pass with the double radius r
template <typename T>
DICP_HD T iss_ball_R(double r) { return ball_R<T>(iss_ball_grid_radius<T>(r)); }

// Every slot j < P.cnt of the cells cell(fl(p_d - R)) .. cell(fl(p_d + R)) of the grid, in ascending slot order, each once: visit(j)
// returns true to stop the walk.  keys(j): the sorted key of slot j.  -> the number of slots visited.
template <typename T, typename Keys, typename Visit>
DICP_HD unsigned iss_ball_scan(const BallPlan<T>& P, T R, T x, T y, T z, const Keys& keys, const Visit& visit) {
    unsigned visited = 0u;
    const int cnt = P.cnt;
    if (cnt <= 0) return visited;
    if (P.flat) {
        for (int j = 0; j < cnt; ++j) { ++visited; if (visit(j)) break; }
        return visited;
    }
    int64_t lo[3], hi[3];
    if (!ball_range_at(P, R, x, y, z, lo, hi)) return visited;
    const uint64_t ymask = vox_shl(1, P.wy) - 1;
    int64_t cx = lo[0], cy = lo[1];
    while (cx <= hi[0]) {
        const uint64_t k_lo = ball_key(P, cx, cy, lo[2]), k_hi = ball_key(P, cx, cy, hi[2]);
        int j = ball_lower_bound(keys, cnt, k_lo);
        if (j >= cnt) break;
        const uint64_t kj = keys(j);
        if (kj <= k_hi) {
            bool stop;
            do { ++visited; stop = visit(j); ++j; } while (!stop && j < cnt && keys(j) <= k_hi);
            if (stop) break;
        } else {
            const uint64_t col = kj >> P.wz;                // the column of the first row past this one: (kx, ky) >= (cx, cy)
            const int64_t kx = (int64_t)(col >> P.wy), ky = (int64_t)(col & ymask);
            if (kx > cx || ky > cy) {                       // jump to that column, or past it where it lies outside the range
                const int64_t ty = kx > cx ? (ky < lo[1] ? lo[1] : ky) : ky;
                cx = kx;
                if (ty > hi[1]) { ++cx; cy = lo[1]; } else cy = ty;
                continue;
            }
        }
        if (++cy > hi[1]) { ++cx; cy = lo[1]; }
    }
    return visited;
}

template <typename V>
DICP_HD void iss_ball_load(const V& v, double* p) { p[0] = (double)v.x; p[1] = (double)v.y; p[2] = (double)v.z; }

// Pass 1 of the live row in sorted slot s: row(j) the packed row of slot j (.x .y .z of T).  -> l[3], the double saliency; count and
// the slots visited by the two walks through the references.
template <typename T, typename Keys, typename Row>
DICP_HD double iss_ball_saliency_row(const BallPlan<T>& P, T R, double radius2, int s, const Keys& keys, const Row& row, double gamma21,
                                     double gamma32, int min_neighbors, double* l, int& count, unsigned& visited) {
    const auto self = row(s);
    double pi[3];
    iss_ball_load(self, pi);
    double sum[3] = {0.0, 0.0, 0.0};
    int n = 1;                                              // the row itself: q = 0 adds nothing to the sum
    visited = iss_ball_scan<T>(P, R, (T)self.x, (T)self.y, (T)self.z, keys, [&](int j) {
        if (j == s) return false;
        double pj[3], q[3];
        iss_ball_load(row(j), pj);
        const double r2 = iss_d2(pi, pj, q);
        if (iss_member(true, r2, radius2)) { ++n; iss_mean_add(sum, q); }
        return false;
    });
    double mu[3], a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double zero[3] = {0.0, 0.0, 0.0};
    iss_mean(sum, n, mu);
    iss_cov_add(a, zero, mu);
    visited += iss_ball_scan<T>(P, R, (T)self.x, (T)self.y, (T)self.z, keys, [&](int j) {
        if (j == s) return false;
        double pj[3], q[3];
        iss_ball_load(row(j), pj);
        const double r2 = iss_d2(pi, pj, q);
        if (iss_member(true, r2, radius2)) iss_cov_add(a, q, mu);
        return false;
    });
    iss_cov_scale(a, n);
    iss_eigenvalues(a, l);
    count = n;
    return iss_saliency(l, n, gamma21, gamma32, min_neighbors);
}

// Pass 2 of the live row i in sorted slot s whose double saliency sal_i is > 0: sal(j) the double saliency and orig(j) the row index of
// slot j.  -> is it a keypoint?  The walk stops at the first member that beats the row.
template <typename T, typename Keys, typename Row, typename Sal, typename Orig>
DICP_HD bool iss_ball_maximum_row(const BallPlan<T>& P, T R, double radius2, int s, int i, double sal_i, int min_neighbors, const Keys& keys,
                                  const Row& row, const Sal& sal, const Orig& orig, unsigned& visited) {
    const auto self = row(s);
    double pi[3];
    iss_ball_load(self, pi);
    int n = 1;
    bool beaten = false;
    visited = iss_ball_scan<T>(P, R, (T)self.x, (T)self.y, (T)self.z, keys, [&](int j) {
        if (j == s) return false;
        double pj[3], q[3];
        iss_ball_load(row(j), pj);
        const double r2 = iss_d2(pi, pj, q);
        if (!iss_member(true, r2, radius2)) return false;
        ++n;
        beaten = iss_beats(sal(j), orig(j), sal_i, i);
        return beaten;
    });
    return !beaten && n >= min_neighbors;
}

}  // namespace dicp
