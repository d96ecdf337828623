// Graduated non-convexity over explicit correspondences (dicp_amd/match.py: gnc_correspondences): the per-element rules, the order of
// the sums and the stopping rules of csrc/gnc.hip.
//
// Plain inline C++ templated on the scalar T, included by the HIP kernel and by a TEST-ONLY g++ build (tests/test_gnc_host.py) that runs
// the same lines in a serial loop and holds them to the numpy restatement tests/gnc_ref.py.
//
// Everything is in double; float inputs are converted exactly.  The only operations are + - * / sqrt and comparisons: no fma, no libm.
// The build contracts a * b + c only inside ONE expression (-ffp-contract=on): every product that is added to something is a statement of
// its own here, and csrc/gnc.hip switches contraction off for its whole translation unit, so that kabsch_forward (dicp_math.h) rounds on
// the device as it does in the g++ build.
//
// A cloud's live pairs are packed (x[0:3], y[0:3]) rows of 6 values of T, P of them, in ascending row order; u_p is the user weight of
// pair p (1 without one).  c2 = threshold threshold, g = growth.
//   residual under a pose (C row-major, r) in double:  q_a = ((C_a0 x_0 + C_a1 x_1) + C_a2 x_2) + r_a,  e_a = q_a - y_a,
//       d = (e_0 e_0 + e_1 e_1) + e_2 e_2;  a d that is not finite counts as +inf.
//   weight of a round at mu:
//       TLS  lo = (mu / (mu + 1)) c2,  hi = ((mu + 1) / mu) c2:  w = 1 for d <= lo,  0 for d >= hi (and for +inf),  and in the band
//            w = sqrt(((c2 mu) (mu + 1)) / d) - mu, clamped into [0, 1] (the clamp only ever moves a last bit)
//       GM   t = mu c2,  q = t / (d + t),  w = q q;  0 for +inf
//       a w that is not > 0 is stored as 0.  omega_p = u_p w_p, and only pairs with omega_p > 0 enter a fit.
//   the 18 sums F(w): slot s = p mod GNC_SLOTS takes its pairs p = s, s + GNC_SLOTS, ... in ascending p from +0 (gnc_add), then the
//       slots are added pairwise, v_i = v_i + v_(i + off) for off = 1, 2, 4, ... and every i that is a multiple of 2 off (gnc_tree): one fixed
//       tree, a function of P alone.  Then kabsch_forward (proper rotation, rank-deficient completion); the pose stays in double.
//   round 0: w = 1, pose = F(w), d under it, dmax = the largest finite d (0 when there is none).
//   start (gnc_begin):  TLS: 2 dmax <= c2 stops at once, status 0; otherwise mu = c2 / (2 dmax - c2).   GM: mu = max(1, 2 dmax / c2).
//   a round (gnc_apply): weights from the d of the current pose at mu; with fewer than three omega_p > 0 the round is NOT applied (the
//       previous pose and weights stand) and the loop stops, status 2.  Otherwise pose = F(w), rounds += 1, and the loop stops with
//       status 0 when the band was empty (TLS) / mu was 1 (GM), else with status 1 when rounds == iterations, else
//       mu = mu g (TLS) / max(1, mu / g) (GM).
//   P < 3: nothing runs; weights 0, rounds 0, status 3, mu 0, the identity pose.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dicp_math.h"

namespace dicp {

constexpr int GNC_SLOTS = 1024;         // slots of the sums' tree = lanes of the kernel's workgroup
constexpr int GNC_ROW = 6;              // values of a packed pair: x[0:3], y[0:3]
constexpr int GNC_ITER_MAX = 256;
constexpr int GNC_TRACE = 32;           // doubles of a trace record: mu, band count, the 18 sums, the pose (12)
constexpr int GNC_TLS = 0, GNC_GM = 1;
constexpr int GNC_CONVERGED = 0, GNC_CAPPED = 1, GNC_GUARDED = 2, GNC_TOO_FEW = 3;

DICP_HD double gnc_inf() { return __builtin_huge_val(); }
DICP_HD bool gnc_finite(double v) { return v - v == 0.0; }

// d of a packed pair under the pose (C row-major, then r) in double; +inf when it is not finite
template <typename T>
DICP_HD double gnc_residual(const double* pose, const T* row) {
    const double x0 = (double)row[0], x1 = (double)row[1], x2 = (double)row[2];
    double d = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double t0 = pose[3 * a] * x0;
        const double t1 = pose[3 * a + 1] * x1;
        const double t2 = pose[3 * a + 2] * x2;
        const double s01 = t0 + t1;
        const double s = s01 + t2;
        const double q = s + pose[9 + a];
        const double e = q - (double)row[3 + a];
        const double ee = e * e;
        d = a == 0 ? ee : d + ee;
    }
    return gnc_finite(d) ? d : gnc_inf();
}

struct GncRound {                       // what every pair of a round sees
    int loss;
    double mu, c2, lo, hi, num, t;
};

DICP_HD GncRound gnc_round(int loss, double mu, double c2) {
    GncRound r;
    r.loss = loss; r.mu = mu; r.c2 = c2;
    const double m1 = mu + 1.0;
    const double a = mu / m1;
    const double b = m1 / mu;
    const double cm = c2 * mu;
    r.lo = a * c2;
    r.hi = b * c2;
    r.num = cm * m1;
    r.t = mu * c2;
    return r;
}

// w of a pair; band = 1 when a TLS pair lies strictly between lo and hi
DICP_HD double gnc_weight(const GncRound& r, double d, int& band) {
    band = 0;
    double w;
    if (!(d < gnc_inf())) {
        w = 0.0;
    } else if (r.loss == GNC_TLS) {
        if (d <= r.lo) {
            w = 1.0;
        } else if (d >= r.hi) {
            w = 0.0;
        } else {
            band = 1;
            const double q = r.num / d;
            w = sqrt(q) - r.mu;
            w = w > 1.0 ? 1.0 : w;
        }
    } else {
        const double den = d + r.t;
        const double q = r.t / den;
        w = q * q;
    }
    return w > 0.0 ? w : 0.0;
}

// one packed pair into the 18 sums at weight omega > 0
template <typename T>
DICP_HD void gnc_add(double* acc, double omega, const T* row) {
    const double p[3] = {(double)row[0], (double)row[1], (double)row[2]};
    const double y[3] = {(double)row[3], (double)row[4], (double)row[5]};
    acc[KAB_S0] = acc[KAB_S0] + omega;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double wp = omega * p[a];
        const double wy = omega * y[a];
        acc[KAB_SP + a] = acc[KAB_SP + a] + wp;
        acc[KAB_SY + a] = acc[KAB_SY + a] + wy;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double m = wy * p[b];
            acc[KAB_M + a * 3 + b] = acc[KAB_M + a * 3 + b] + m;
        }
    }
    const double p0 = p[0] * p[0], p1 = p[1] * p[1], p2 = p[2] * p[2];
    const double y0 = y[0] * y[0], y1 = y[1] * y[1], y2 = y[2] * y[2];
    const double p01 = p0 + p1, y01 = y0 + y1;
    const double pp = p01 + p2, yy = y01 + y2;
    const double wpp = omega * pp, wyy = omega * yy;
    acc[KAB_PP] = acc[KAB_PP] + wpp;
    acc[KAB_YY] = acc[KAB_YY] + wyy;
}

// the pairwise tree over `count` (a power of two) values `stride` doubles apart; the total ends in v[0]
DICP_HD void gnc_tree_one(double* v, int count, int stride) {
    for (int off = 1; off < count; off <<= 1)
        for (int i = 0; i < count; i += 2 * off) v[(size_t)i * stride] = v[(size_t)i * stride] + v[(size_t)(i + off) * stride];
}

// ... over `count` records of NKAB sums, `stride` doubles apart; the totals end in record 0.  The kernel runs the levels below a wave's
// 64 slots as a butterfly over the lanes (a + b is b + a bit for bit) and the levels above with gnc_tree_one, a lane per sum.
DICP_HD void gnc_tree(double* v, int count, int stride) {
    for (int k = 0; k < NKAB; ++k) gnc_tree_one(v + k, count, stride);
}

struct GncState {
    double mu;              // of the next round
    double mu_used;         // of the last applied round, 0 if none
    int32_t rounds, status, go;
};

// after round 0
DICP_HD void gnc_begin(int loss, double dmax, double c2, GncState& s) {
    s.rounds = 0; s.status = GNC_CONVERGED; s.go = 1; s.mu_used = 0.0;
    const double two = 2.0 * dmax;
    if (loss == GNC_TLS) {
        if (two <= c2) { s.go = 0; s.mu = 0.0; return; }
        s.mu = c2 / (two - c2);
    } else {
        const double q = two / c2;
        s.mu = q > 1.0 ? q : 1.0;
    }
}

// after the weights of a round at s.mu: npos pairs with omega > 0, band pairs in the TLS band -> is the round applied?
DICP_HD bool gnc_apply(int loss, int64_t npos, int64_t band, double growth, int iterations, GncState& s) {
    if (npos < 3) { s.status = GNC_GUARDED; s.go = 0; return false; }
    s.rounds += 1;
    s.mu_used = s.mu;
    const bool done = loss == GNC_TLS ? band == 0 : !(s.mu > 1.0);
    if (done) { s.status = GNC_CONVERGED; s.go = 0; }
    else if (s.rounds >= iterations) { s.status = GNC_CAPPED; s.go = 0; }
    else if (loss == GNC_TLS) { s.mu = s.mu * growth; }
    else { const double q = s.mu / growth; s.mu = q > 1.0 ? q : 1.0; }
    return true;
}

DICP_HD bool gnc_bad_arguments(int loss, double threshold, double growth, int iterations) {
    const double c2 = threshold * threshold;
    return !(loss == GNC_TLS || loss == GNC_GM) || !(threshold > 0.0 && c2 > 0.0 && c2 < gnc_inf()) || !(growth > 1.0 && growth <= 16.0) ||
           iterations < 1 || iterations > GNC_ITER_MAX;
}

}  // namespace dicp
