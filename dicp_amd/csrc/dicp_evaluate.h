// Registration quality of candidate poses (dicp_amd/evaluate.py: evaluate_registration, information_matrix): the per-row rules and the
// order of the sums of csrc/evaluate.hip.
//
// Plain inline C++ templated on the scalar T, included by the HIP kernels and by a TEST-ONLY g++ build (tests/test_evaluate_host.py) that
// runs the same lines in a serial loop over a host-built grid and holds them to the numpy restatement tests/evaluate_ref.py.
//
// T is the points' dtype.  "double" means on exactly converted values with + - * / sqrt only and no fma: every product that is added to
// something is a statement of its own (the build contracts a * b + c only inside ONE expression).
//   1 pose      of (cloud b, hypothesis h): C_ak = T[b,h,a,k], r_a = T[b,h,a,3] -- rows 0:3 of the 4x4 matrix, read in T.
//   2 query     q_a = fma(C_a2, x_2, fma(C_a1, x_1, fma(C_a0, x_0, r_a))) in T (ransac_residual's chain, match_fma).  Source row i is a
//               QUERY under the pose when i < source_rows[b] and q_0, q_1, q_2 are finite.
//   3 match     slot 0 of ball_query(q, target, max_distance, k = 1, y_rows = target_rows), exactly: the candidates are the target rows
//               j < target_rows[b] with finite coordinates and d2 = topk_d2(q, y_j) <= r2, r2 = max_distance rounded to T then squared
//               in T; the winner is the first in (d2, j) order; without a candidate idx = -1 and d2 = +inf.
//   4 count     the number of matched queries; fitness = count / source_rows[b] in double (n without row counts), 0 for a cloud
//               with no rows.
//   5 terms     a matched row has ten double terms, with t = (double) y_match:  e = (double) d2;  t_x, t_y, t_z;
//               t_x t_x, t_y t_y, t_z t_z, t_x t_y, t_x t_z, t_y t_z.  Every other row contributes +0 to each.
//   6 order     of every sum, a function of n alone: tile c holds rows 256 c .. 256 c + 255 (rows at or past n contribute +0); within a
//               tile v_l = v_l + v_(l + off) for off = 1, 2, 4, .., 128 and every l that is a multiple of 2 off (eval_tile_tree: the
//               pairwise tree of gnc_correspondences); the tile results are added in ascending c to a total that starts at +0.
//   7 rmse      inlier_rmse = sqrt(SSE / count) in double, 0 when count = 0.
//   8 matrix    Open3D's sum of G^T G over the matched target points, G = [-[t]x | I] (rotation first), assembled from the nine moment
//               sums in torch (dicp_amd/evaluate.py); the sign of a zero entry is not part of the definition.
// A non-finite pose leaves no finite q, an empty target no candidate, a source without rows no query: count 0, fitness 0, rmse 0 and
// zero sums all follow from the rules above.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "dicp_ball.h"
#include "dicp_match.h"

namespace dicp {

constexpr int EVAL_TILE = 256;          // rows of a tile = lanes of the kernel's workgroup
constexpr int EVAL_TERMS = 10;          // e, t (3), the six second moments
constexpr int EVAL_H_MAX = 65536;
// the terms' slots
constexpr int EVAL_E = 0, EVAL_T = 1, EVAL_XX = 4, EVAL_YY = 5, EVAL_ZZ = 6, EVAL_XY = 7, EVAL_XZ = 8, EVAL_YZ = 9;

DICP_HD int eval_tiles(int n) { return (n + EVAL_TILE - 1) / EVAL_TILE; }

// rule 1: the 12 values of a pose from the 16 of its row-major 4x4 matrix: C row-major, then r
template <typename T>
DICP_HD void eval_load_pose(const T* m44, T (&pose)[12]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        pose[3 * a] = m44[4 * a]; pose[3 * a + 1] = m44[4 * a + 1]; pose[3 * a + 2] = m44[4 * a + 2];
        pose[9 + a] = m44[4 * a + 3];
    }
}

template <typename T> struct EvalPoint { T x, y, z; };

// rule 2: false when a coordinate of q is not finite
template <typename T>
DICP_HD bool eval_query(const T (&pose)[12], T x0, T x1, T x2, EvalPoint<T>& q) {
    q.x = match_fma(pose[2], x2, match_fma(pose[1], x1, match_fma(pose[0], x0, pose[9])));
    q.y = match_fma(pose[5], x2, match_fma(pose[4], x1, match_fma(pose[3], x0, pose[10])));
    q.z = match_fma(pose[8], x2, match_fma(pose[7], x1, match_fma(pose[6], x0, pose[11])));
    return ball_finite(q.x) && ball_finite(q.y) && ball_finite(q.z);
}

// rule 3: the best candidate so far: (d2, original index) and the sorted slot it came from; empty: (+inf, -1, -1)
template <typename T>
struct EvalBest { T d2; int idx; int slot; };

template <typename T>
DICP_HD void eval_best_init(EvalBest<T>& b) { b.d2 = static_cast<T>(__builtin_huge_val()); b.idx = -1; b.slot = -1; }

// The best-of-one inserter of ball_scan: ins(d2, j) for slot j of the sorted cloud with a finite d2 <= r2; orig(j) its original index,
// read only when d2 can enter.  Ties in d2 go to the lower original index.
template <typename T, typename Orig>
DICP_HD auto eval_inserter(EvalBest<T>& b, const Orig& orig) {
    return [&b, &orig](T d2, int j) {
        if (!(d2 <= b.d2)) return;
        const int o = orig(j);
        if (d2 < b.d2 || o < b.idx) { b.d2 = d2; b.idx = o; b.slot = j; }            // (d2 == b.d2 is finite: b holds a row)
    };
}

// rule 5: the ten terms of a row; y: the matched target row (.x .y .z), not examined when the row has no match
template <typename T, typename Y>
DICP_HD void eval_terms(bool matched, T d2, const Y& y, double (&v)[EVAL_TERMS]) {
    if (!matched) {
#pragma unroll
        for (int k = 0; k < EVAL_TERMS; ++k) v[k] = 0.0;
        return;
    }
    const double tx = (double)y.x, ty = (double)y.y, tz = (double)y.z;
    v[EVAL_E] = (double)d2;
    v[EVAL_T] = tx; v[EVAL_T + 1] = ty; v[EVAL_T + 2] = tz;
    const double xx = tx * tx, yy = ty * ty, zz = tz * tz;
    const double xy = tx * ty, xz = tx * tz, yz = ty * tz;
    v[EVAL_XX] = xx; v[EVAL_YY] = yy; v[EVAL_ZZ] = zz;
    v[EVAL_XY] = xy; v[EVAL_XZ] = xz; v[EVAL_YZ] = yz;
}

// rule 6 within a tile: the pairwise tree over `count` (a power of two) values `stride` doubles apart; the total ends in v[0].  The
// kernel runs the levels below a wave's 64 lanes as a butterfly (a + b is b + a bit for bit) and the two above through LDS.
DICP_HD void eval_tile_tree(double* v, int count, int stride) {
    for (int off = 1; off < count; off <<= 1)
        for (int i = 0; i < count; i += 2 * off) v[(size_t)i * stride] = v[(size_t)i * stride] + v[(size_t)(i + off) * stride];
}

// rule 6 across tiles: `tiles` records `stride` doubles apart, added in ascending order to a total that starts at +0
DICP_HD double eval_join_tiles(const double* rec, int tiles, size_t stride) {
    double s = 0.0;
    for (int c = 0; c < tiles; ++c) s = s + rec[(size_t)c * stride];
    return s;
}

// rule 4
DICP_HD double eval_fitness(int32_t count, int32_t rows) {
    if (rows <= 0) return 0.0;
    return (double)count / (double)rows;
}

// rule 7
DICP_HD double eval_rmse(double sse, int32_t count) {
    if (count <= 0) return 0.0;
    const double q = sse / (double)count;
    return sqrt(q);
}

}  // namespace dicp
