// The cell grid of one cloud and the fixed-radius scan over it (dicp_amd/ball.py: ball_query; csrc/ball_query.hip).
//
// Plain inline C++ templated on the scalar T and on accessors, included by the HIP kernels and by a TEST-ONLY g++ build
// (tests/test_ball_host.py) that holds the cell arithmetic, the plan, the keys, the range enumeration and
// the per-query scan to a numpy brute force.
//
// The grid of a cloud: its rows j < rows[b] with three finite coordinates ("live" rows), sorted by a 64-bit cell key.  With the origin o
// (the live rows' per-axis minimum) and the per-axis cell edge s,
//   cell_d(a) = floor(fl(fl(a - o_d) / s_d))                 dicp_voxel.h's vox_coord: one rounded subtraction, one IEEE division, floor
//   key = (cx << (w_y + w_z)) | (cy << w_z) | cz             lexicographic (cx, cy, cz); w_d = bit_length(cell_d(max_d)), w_x+w_y+w_z <= 63
// (63, not 64, so that no live key is the all-ones key of the rows that stay out of the grid and of the sort's padding).
//
// The candidates of a query p are the live rows y with d2 = topk_d2(p, y) <= r2 = fl(radius * radius) (d2 finite).
// CLAIM: with R = ball_R(radius) every candidate has, on every axis d,
//   cell_d(fl(p_d - R)) <= cell_d(y_d) <= cell_d(fl(p_d + R)).
// So the scan visits those cells (intersected with the grid's cells 0 .. hi_d) whatever number of them that is -- not "27 cells": with
// s = R the range spans up to 4 cells per axis in float32 (3 in float64), and more where the rounding of p +- R is coarser than s.
// PROOF.  u is the unit roundoff (2^-24 / 2^-53), eta the smallest subnormal (2^-149 / 2^-1074).
//  (1) d2 = fl(fl(xx + yy) + zz) >= xx: the terms are non-negative and rounding is monotone.  So a candidate has xx <= r2, with
//      xx = fl(e * e), e = fl(y_d - p_d) (the same for yy and zz).
//  (2) A rounded product is within a factor (1 +- u) of the exact one or, where it underflows, within eta / 2 of it:
//      xx >= e^2 (1 - u) - eta / 2 and r2 <= radius^2 (1 + u) + eta / 2.  Hence e^2 (1 - u) <= radius^2 (1 + u) + eta and
//      |e| <= radius * a + b with a = sqrt((1 + u) / (1 - u)) <= 1 + 2u and b = sqrt(eta / (1 - u)) <= 1.01 sqrt(eta).
//  (3) A rounded difference is exact where it is subnormal and within (1 +- u) otherwise: |y_d - p_d| <= |e| / (1 - u) in exact reals.
//  (4) If radius >= b / u then radius * a + b <= radius (1 + 3u), and |y_d - p_d| <= radius (1 + 3u) / (1 - u) <= radius (1 + 5u).
//      ball_R takes fl(radius * (1 + 8u)) >= radius (1 + 8u)(1 - u) >= radius (1 + 6u) (the product is normal here) and the next float up.
//      Otherwise radius * a + b < b (a / u + 1) < 1.1 sqrt(eta) / u, and |y_d - p_d| < 1.2 sqrt(eta) / u <= BallFloor = 2^-49 / 2^-483
//      (sqrt(eta) / u = 2^-50.5 / 2^-484: of the order of sqrt(smallest normal) / sqrt(u)).  The float32 radius 1e-25 has r2 = 0, and
//      a row 1e-23 away has d2 = 0 and is a candidate: it is inside the floor.  ball_R is the larger of the two.
//      (r2 = +inf for a large radius makes every live row a candidate; R is then huge or +inf and the range is the whole grid.)
//  (5) So p_d - R <= y_d <= p_d + R in exact reals; y_d is a number of T and rounding is monotone: fl(p_d - R) <= y_d <= fl(p_d + R).
//  (6) cell_d is monotone (non-decreasing) in its argument: a rounded subtraction of a constant, a rounded division by a positive
//      constant and floor all are.  ball_cell is cell_d saturated at +-2^62, which keeps it monotone, and is defined for +-inf.  QED.
// The live rows lie in cells 0 .. hi_d (o_d <= y_d <= max_d and (6)), so the intersection loses nothing; a query far outside the cloud,
// or past the convertible range, has an empty intersection and no neighbours.
//
// The plan (ball_plan): s starts at R on every axis.  An axis whose cell_d(max_d) is not below 2^62 gets its edge multiplied by 2^30 until
// it is; then, while the widths exceed 63 bits in total, the widest axis' edge is doubled.  Larger cells stay correct (the claim holds for
// any s > 0), only slower.  At most 2^2098 / 2^30 steps of the first kind (70) and 3 * 62 of the second; a cloud that still does not fit
// -- an extent that overflows T, an infinite R -- is "flat": one cell, every key 0, every query scans every live row.  A radius that is
// not a finite number > 0 (it can only arrive so from device memory; the Python layer refuses it) gives a grid with no live rows.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dicp_math.h"
#include "dicp_topk.h"
#include "dicp_voxel.h"

namespace dicp {

constexpr int BALL_KEY_BITS = 63;
constexpr uint64_t BALL_NO_KEY = ~(uint64_t)0;          // rows that stay out of the grid, and the padding of the sort
constexpr int BALL_PLAN_STEPS = 512;
constexpr int64_t BALL_SAT = (int64_t)1 << 62;

template <typename T> struct BallNum;
template <> struct BallNum<float> {
    static constexpr float grow = 1.0f + 0x1p-20f;          // 1 + 8u
    static constexpr float floor_R = 0x1p-49f;
};
template <> struct BallNum<double> {
    static constexpr double grow = 1.0 + 0x1p-50;           // 1 + 8u
    static constexpr double floor_R = 0x1p-483;
};

DICP_HD float  ball_next_up(float x)  { return nextafterf(x, __builtin_huge_valf()); }
DICP_HD double ball_next_up(double x) { return nextafter(x, __builtin_huge_val()); }

template <typename T>
DICP_HD bool ball_finite(T x) { return x - x == T(0); }                // false for inf and NaN

// The search half-width of the proof above
template <typename T>
DICP_HD T ball_R(T radius) {
    const T g = radius * BallNum<T>::grow;
    const T R = ball_next_up(g);
    return R > BallNum<T>::floor_R ? R : BallNum<T>::floor_R;
}

// floor((a - o) / s) in T saturated at +-2^62; false (and 0) for a NaN
template <typename T>
DICP_HD bool ball_cell(T a, T o, T s, int64_t* v) {
    const T d = a - o;
    const T q = d / s;
    const double f = (double)vox_floor(q);
    if (f != f) { *v = 0; return false; }
    *v = f >= VOX_COORD_LIMIT ? BALL_SAT : (f <= -VOX_COORD_LIMIT ? -BALL_SAT : (int64_t)f);
    return true;
}

template <typename T>
struct BallPlan {
    T o[3], s[3];               // origin and cell edge per axis
    T R, r2;                    // search half-width, fl(radius * radius)
    int64_t hi[3];              // the live rows lie in cells 0 .. hi[d]
    int32_t wy, wz;             // key widths of cy and cz
    int32_t cnt;                // live rows: the first cnt sorted slots
    int32_t flat;               // 1: one cell (hi = 0), queries scan every live row
};
constexpr int BALL_PLAN_BYTES = 128;                    // one plan per cloud in device memory, this far apart

// mn, mx: the per-axis bounds of the cnt live rows of the cloud (unused when cnt = 0)
template <typename T>
DICP_HD BallPlan<T> ball_plan(const T* mn, const T* mx, int cnt, T radius) {
    BallPlan<T> P;
    const bool ok = radius > T(0) && ball_finite(radius);
    P.R = ok ? ball_R(radius) : T(0);
    P.r2 = ok ? radius * radius : T(0);
    P.cnt = ok ? cnt : 0;
    P.flat = 1;
    P.wy = P.wz = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) { P.o[d] = P.cnt ? mn[d] : T(0); P.s[d] = P.R; P.hi[d] = 0; }
    if (!P.cnt || !ball_finite(P.R)) return P;
    int w[3] = {0, 0, 0};
    for (int it = 0; it < BALL_PLAN_STEPS; ++it) {
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
        if (w[0] >= w[1] && w[0] >= w[2]) P.s[0] = P.s[0] * T(2);         // (no indexing by a variable: the plan stays in registers)
        else if (w[1] >= w[2]) P.s[1] = P.s[1] * T(2);
        else P.s[2] = P.s[2] * T(2);
    }
    if (P.flat) { for (int d = 0; d < 3; ++d) P.hi[d] = 0; return P; }
    P.wy = w[1];
    P.wz = w[2];
    return P;
}

template <typename T>
DICP_HD bool ball_enlarged(const BallPlan<T>& P) { return P.flat || P.s[0] != P.R || P.s[1] != P.R || P.s[2] != P.R; }

template <typename T>
DICP_HD uint64_t ball_key(const BallPlan<T>& P, int64_t cx, int64_t cy, int64_t cz) {
    return vox_shl((uint64_t)cx, P.wy + P.wz) | vox_shl((uint64_t)cy, P.wz) | (uint64_t)cz;
}

DICP_HD int64_t ball_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The key of a live row of the grid's own cloud (its cells are 0 .. hi by monotonicity; the clamp is a belt for the key's width), and,
// for a finite point of another cloud, the key of the grid cell nearest to it: the order the queries are processed in.
template <typename T>
DICP_HD uint64_t ball_point_key(const BallPlan<T>& P, T x, T y, T z) {
    if (P.flat) return 0;
    const T p[3] = {x, y, z};
    int64_t c[3];
    for (int d = 0; d < 3; ++d) {
        if (!ball_cell(p[d], P.o[d], P.s[d], &c[d])) return BALL_NO_KEY;
        c[d] = ball_clamp(c[d], P.hi[d]);
    }
    return ball_key(P, c[0], c[1], c[2]);
}

// The cells cell(fl(p_d - R)) .. cell(fl(p_d + R)) intersected with 0 .. hi_d; false when the intersection is empty on some axis.
// ball_range_at takes the half-width as an argument (dicp_gridknn.h searches one grid at several), ball_range the plan's own.
template <typename T>
DICP_HD bool ball_range_at(const BallPlan<T>& P, T R, T x, T y, T z, int64_t* lo, int64_t* hi) {
    const T p[3] = {x, y, z};
    for (int d = 0; d < 3; ++d) {
        const T a = p[d] - R;
        const T b = p[d] + R;
        if (!ball_cell(a, P.o[d], P.s[d], &lo[d]) || !ball_cell(b, P.o[d], P.s[d], &hi[d])) return false;
        if (lo[d] < 0) lo[d] = 0;
        if (hi[d] > P.hi[d]) hi[d] = P.hi[d];
        if (lo[d] > hi[d]) return false;
    }
    return true;
}

template <typename T>
DICP_HD bool ball_range(const BallPlan<T>& P, T x, T y, T z, int64_t* lo, int64_t* hi) { return ball_range_at(P, P.R, x, y, z, lo, hi); }

// The first of keys[0, n) (ascending) that is not below k; n when there is none
template <typename Keys>
DICP_HD int ball_lower_bound(const Keys& keys, int n, uint64_t k) {
    int lo = 0, len = n;
    while (len > 0) {
        const int h = len >> 1;
        if (keys(lo + h) < k) { lo += h + 1; len -= h + 1; }
        else len = h;
    }
    return lo;
}

struct BallScan { int count; unsigned visited; int spans[3]; };

// The scan of one query p (three finite coordinates) over a grid: keys(j) / row(j) the sorted key and row of slot j < P.cnt; every
// live row of the visited cells goes through topk_d2, d2 <= r2 bumps the count and feeds ins(d2, j).
// For a fixed column (cx, cy) the cells cz_lo .. cz_hi are adjacent in the key: one contiguous range of slots, found by a binary search
// for its first key and left when a key passes its last.  A column without rows is not searched again: the key the search lands on names
// the next column that has any, and the scan jumps there.  Every pass of the outer loop moves (cx, cy) forward and, but for one pass
// after each jump, lands on a row not seen before: at most 3 cnt + 2 passes, each a search of log2(cnt) steps, and at most cnt rows
// scanned in all -- bounded by the cloud's row count whatever the coordinates are.
template <typename T, typename Q, typename Keys, typename Row, typename Ins>
DICP_HD BallScan ball_scan(const BallPlan<T>& P, const Q& p, const Keys& keys, const Row& row, const Ins& ins) {
    BallScan out = {0, 0u, {0, 0, 0}};
    const int cnt = P.cnt;
    if (cnt <= 0) return out;
    auto visit = [&](int j) {
        const T d2 = topk_d2<T>(p, row(j));
        ++out.visited;
        if (d2 <= P.r2 && d2 < static_cast<T>(__builtin_huge_val())) { ++out.count; ins(d2, j); }      // (false for a NaN d2)
    };
    if (P.flat) {
        for (int j = 0; j < cnt; ++j) visit(j);
        return out;
    }
    int64_t lo[3], hi[3];
    if (!ball_range(P, (T)p.x, (T)p.y, (T)p.z, lo, hi)) return out;
    for (int d = 0; d < 3; ++d) out.spans[d] = (int)(hi[d] - lo[d] + 1 > 0x7fffffff ? 0x7fffffff : hi[d] - lo[d] + 1);
    const uint64_t ymask = vox_shl(1, P.wy) - 1;
    int64_t cx = lo[0], cy = lo[1];
    while (cx <= hi[0]) {
        const uint64_t k_lo = ball_key(P, cx, cy, lo[2]), k_hi = ball_key(P, cx, cy, hi[2]);
        int j = ball_lower_bound(keys, cnt, k_lo);
        if (j >= cnt) break;
        uint64_t kj = keys(j);
        if (kj <= k_hi) {
            do { visit(j); ++j; } while (j < cnt && keys(j) <= k_hi);
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
    return out;
}

}  // namespace dicp
