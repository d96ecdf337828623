// The whole-ball neighbour list of the FPFH descriptor (dicp_amd/fpfh.py: fpfh_features_ball / compute_fpfh(whole_ball=True);
// csrc/fpfh_ball.hip): every row of the ball, found by walking the cloud's cell grid (csrc/dicp_ball.h), instead of the k <= 32 slots of
// a neighbour index -- and the descriptor of CHOSEN rows only (`at`).
//
// Plain inline C++ templated on the scalar T of the points and on accessors, included by the HIP kernels and by a TEST-ONLY g++ build
// (tests/test_fpfh_ball_host.py) that holds the walk and the two passes to numpy (tests/fpfh_ball_ref.py) on a CPU box with no GPU.
//
// DEFINITION.  Everything of csrc/dicp_fpfh.h stands and is called unchanged -- fpfh_row_ok, fpfh_d2, fpfh_near, fpfh_pair_bins,
// fpfh_spfh, fpfh_weight, fpfh_weight_add, fpfh_out --; only the neighbour list changes.
//   The grid is ball_query's (dicp_ball_grid_build), built on the points' dtype T at iss_ball_grid_radius<T>(radius).  Its LIVE rows are
//     the rows j < rows[b] with three finite coordinates; an OK row is additionally fpfh_row_ok: a finite, non-zero normal.
//   The NEAR LIST of an OK row i is every OTHER live row j that is OK and has r2 = fpfh_d2(p_i, p_j) > 0 and r2 <= radius2 = fl(radius
//     radius) in double (fpfh_near), in ASCENDING (cell key, row index) ORDER: the order of the sorted slots of the cloud's grid
//     (csrc/dicp_iss_ball.h states it).  Exact duplicates (r2 = 0) are NOT near: FPFH's rule, unlike the members of ISS.
//   Pass 1: over the near list, a near row is a PAIR when fpfh_pair_bins finds its frame; each pair adds 1 to three of the row's 33
//     counters (32-bit: a ball may hold more than 255 pairs).  c_i = the number of pairs, s_i[ch] = fpfh_spfh(cnt[i, ch], c_i).
//   Pass 2: over the near list in that order from +0, acc[ch] = fpfh_weight_add(acc[ch], fpfh_weight(r2), s_j[ch]); then per group of 11
//     channels S = the sum of acc in ascending channel order from +0 and out[ch] = fpfh_out(acc[ch], S, s_i[ch]), rounded once to T.
//   Rows that are not OK, and the dead entries of `at`, get 33 zeros.  An entry a of `at` is live when 0 <= a < rows[b]: one unsigned
//     compare against m (dicp_group.h: group_row), then the inverse map row -> sorted slot, which is -1 for every row outside the grid,
//     the rows at or past rows[b] among them.
//   The table between the passes holds, per sorted slot, the 33 doubles s_j[ch] and the OK flag (FPFH_BALL_ROW doubles): s_j is a pure
//     function of two integers, so forming it once per row gives the bits that forming it once per (row, member) would.
//
// COVERAGE.  The walk is iss_ball_scan (csrc/dicp_iss_ball.h) at the half-width iss_ball_R<T>(radius).  fpfh_d2 is iss_d2 operation for
// operation (the three differences p_j - p_i, the three products rounded, (xx + yy) + zz), and the radius test of fpfh_near, r2 <=
// radius2 with radius2 = fl(radius radius) in double, is iss_member's.  So every row this list admits is a member in the sense of the
// COVERAGE CLAIM of csrc/dicp_iss_ball.h, which proves that iss_ball_scan visits every member, each once, in ascending slot order, with
// at most cnt rows visited whatever the coordinates are.  r2 > 0 and the OK flags only REMOVE rows from that list.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dicp_fpfh.h"
#include "dicp_iss_ball.h"

namespace dicp {

constexpr int FPFH_BALL_ROW = FPFH_CH + 1;                  // doubles per slot of the table: s[0:33], then the OK flag (1.0 / 0.0)

// the sorted slot that entry a of `at` names, -1 for a dead entry.  inv(i): the sorted slot of row i < m, -1 for a row outside the grid
template <typename I, typename Inv>
DICP_HD int fpfh_ball_at(I a, int m, const Inv& inv) {
    const int i = group_row(a, m);
    return i < 0 ? -1 : inv(i);
}

// The near list of the OK row in sorted slot s, in order: near(j, r2, d) for every near slot j, d = p_j - p_i.  row(j): the packed row
// of slot j (.x .y .z of T); ok(j): the OK flag of slot j, asked only of slots inside the radius.  -> the number of slots visited.
template <typename T, typename Keys, typename Row, typename Ok, typename Near>
DICP_HD unsigned fpfh_ball_near_list(const BallPlan<T>& P, T R, double radius2, int s, const Keys& keys, const Row& row, const Ok& ok,
                                     const Near& near) {
    const auto self = row(s);
    double pi[3];
    iss_ball_load(self, pi);
    return iss_ball_scan<T>(P, R, (T)self.x, (T)self.y, (T)self.z, keys, [&](int j) {
        if (j == s) return false;
        double pj[3], d[3];
        iss_ball_load(row(j), pj);
        const double r2 = fpfh_d2(pi, pj, d);
        if (!fpfh_near(true, true, r2, radius2)) return false;          // (the flag of slot j is read only inside the radius)
        if (fpfh_near(true, ok(j), r2, radius2)) near(j, r2, d);
        return false;
    });
}

// Pass 1 of the OK row in sorted slot s with the normal ni: add(ch) once per pair, ch[3] its three channels.  nrm(j, n): the normal of
// slot j into n[3] -> its OK flag.
template <typename T, typename Keys, typename Row, typename Nrm, typename Add>
DICP_HD unsigned fpfh_ball_spfh_row(const BallPlan<T>& P, T R, double radius2, int s, const double* ni, const Keys& keys, const Row& row,
                                    const Nrm& nrm, const Add& add) {
    double nj[3];
    return fpfh_ball_near_list<T>(P, R, radius2, s, keys, row, [&](int j) { return nrm(j, nj); }, [&](int, double r2, double* d) {
        int ch[3];
        if (fpfh_pair_bins(ni, nj, d, r2, ch)) add(ch);
    });
}

// the table row of a slot from its 33 counts: cnt(ch) -> int
template <typename Cnt>
DICP_HD void fpfh_ball_table_row(const Cnt& cnt, bool ok, double* t) {
    int c = 0;
    for (int a = 0; a < FPFH_BINS; ++a) c += cnt(a);                    // every pair has one theta bin: their sum is the number of pairs
    for (int ch = 0; ch < FPFH_CH; ++ch) t[ch] = fpfh_spfh(cnt(ch), c);
    t[FPFH_CH] = ok ? 1.0 : 0.0;
}

// Pass 2 of the OK row in sorted slot s: acc[33] from +0.  tab(j): the table row of slot j (FPFH_BALL_ROW doubles).
template <typename T, typename Keys, typename Row, typename Tab>
DICP_HD unsigned fpfh_ball_combine_row(const BallPlan<T>& P, T R, double radius2, int s, const Keys& keys, const Row& row, const Tab& tab,
                                       double* acc) {
#pragma unroll
    for (int ch = 0; ch < FPFH_CH; ++ch) acc[ch] = 0.0;
    const double* tj = nullptr;
    return fpfh_ball_near_list<T>(P, R, radius2, s, keys, row, [&](int j) { tj = tab(j); return tj[FPFH_CH] != 0.0; },
                                  [&](int, double r2, double*) {
        const double wt = fpfh_weight(r2);
#pragma unroll
        for (int ch = 0; ch < FPFH_CH; ++ch) acc[ch] = fpfh_weight_add(acc[ch], wt, tj[ch]);
    });
}

// the 33 outputs of a row from its sums and its own table row: store(ch, value in double)
template <typename Store>
DICP_HD void fpfh_ball_out(const double* acc, const double* si, const Store& store) {
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        double S = 0.0;
#pragma unroll
        for (int a = 0; a < FPFH_BINS; ++a) S = S + acc[g * FPFH_BINS + a];
#pragma unroll
        for (int a = 0; a < FPFH_BINS; ++a) {
            const int ch = g * FPFH_BINS + a;
            store(ch, fpfh_out(acc[ch], S, si[ch]));
        }
    }
}

}  // namespace dicp
