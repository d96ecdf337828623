// Whole-ball surface normals with a gather backward (dicp_amd/normals.py: estimate_normals_ball; csrc/normals_ball.hip): the normal of
// a row from EVERY row of its ball of radius R, the neighbourhood of iss_saliency_ball and fpfh_features_ball, and the gradient of the
// points as a gather over each row's own ball walk.
//
// Plain inline C++ templated on the scalar T of the points and on accessors, included by the HIP kernels and by a TEST-ONLY g++ build
// (tests/test_normals_ball_host.py) that holds every rule below to numpy (tests/normals_ball_ref.py) bit for bit on a CPU box.
//
// Everything is in double on the exactly converted inputs; the only operations are + - * / sqrt and comparisons, no fma; every product
// that is added to something is a statement of its own (the rule of dicp_iss.h: -ffp-contract=on cannot change a bit).
//
// 1  LIVE rows, MEMBERS and their ORDER are dicp_iss_ball.h's, unchanged: the row itself first, then every other live row with
//    iss_d2 <= fl(R R) (inclusive, duplicates included) in ascending (cell key, row index) order; n_i counts the row itself.  The walk
//    is iss_ball_scan; its coverage proof covers this list.
// 2  MEAN and COVARIANCE are pass 1 of iss_ball_saliency_row operation for operation (walk 1: iss_mean_add, iss_mean; walk 2:
//    iss_cov_add with the row itself first at q = 0; iss_cov_scale): C is the ISS covariance bit for bit.
// 3  EIGEN-SYSTEM: dicp_iss.h's cyclic Jacobi -- the same rotations, order, ISS_SWEEPS and early exit, restated in nbl_rotate so that
//    dicp_iss.h stays as it is -- with the same (c, s) applied to a V that starts as the identity: for each row r of V,
//    (V_rp, V_rq) <- (c V_rp - s V_rq, s V_rp + c V_rq), four rounded products and two sums.  The three (diagonal value, index) pairs
//    are ordered ascending, ties to the lower index: lam and v_0, v_1, v_2, the columns of V.  No renormalisation.  The eigenvalues
//    equal iss_eigenvalues' bit for bit (the same a, the same statements; a sorted triple does not depend on the sorting network).
// 4  NORMAL n = s v_0 with s by nrm_sign's rule on d = viewpoint - p_i, the dot product (v_0x d_x + v_0y d_y) + v_0z d_z at statement
//    level; on exactly 0 the first non-zero component of v_0 is made positive.  Curvature lam_0 / ((lam_0 + lam_1) + lam_2), 0 unless
//    the trace is > 0.  Every output is rounded once to T.
// 5  A row that is not live gets a zero normal, curvature 0, eigenvalues 0, count 0 and no gradient; a live row with
//    n_i < min_neighbors a zero normal and curvature 0, its count and eigenvalues are still reported.
// 6  GRADIENT.  Row i has a record of NRM_REC = 13 doubles in dicp_normals_det.h's layout: G6 = nrm_grad_cov(lam, v, s, gn, gk, tau),
//    mu_i, p_i, f_i = 2 / n_i; f_i = 0 with G6 = mu = 0 where the row contributes nothing (not live, n_i < min_neighbors, both
//    cotangents absent or all zero, eigenvalues not separated, zero trace).  Row j receives, per component a,
//      grad_j[a] = T( sum_i t_a(i, j) ),   t_a = f_i ((G_a0 d_0 + G_a1 d_1) + G_a2 d_2),   d_c = (p_j,c - p_i,c) - mu_i,c
//    over the members i of j IN j'S OWN MEMBER ORDER (j first), in double from +0 by plain additions, rounded once to T; the statements
//    of nrm_det_term without its rounding to T; a member with f_i = 0 is skipped.
//    SYMMETRY.  The exact derivative sums over the rows i whose ball holds j.  That is the same set: iss_d2(p_i, p_j) and
//    iss_d2(p_j, p_i) are the same double bit for bit -- fl(a - b) = -fl(b - a) and the squares of x and -x are equal, the sums are
//    taken in the same order -- so j is in ball(i) exactly when i is in ball(j).  Hence the gather needs no neighbour index, no
//    inverted index, no atomics and no zero fill, and is bit-reproducible by construction.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dicp_iss_ball.h"
#include "dicp_normals.h"
#include "dicp_normals_det.h"

namespace dicp {

// The state a row's forward leaves for the records pass, so that it does not walk again: NBL_STATE doubles, element e of sorted slot s
// of cloud b at ((b NBL_STATE + e) P + s) (P = the slots of a cloud: consecutive lanes store consecutive doubles):
//   [0..6) the scaled covariance C6, [6..9) mu, [9] n_i, [10] s (+-1), or 0 where n_i < min_neighbors.
constexpr int NBL_STATE = 11;
enum { NBL_C = 0, NBL_MU = 6, NBL_N = 9, NBL_S = 10 };

// iss_rotate with the rotation also applied to the columns P, Q of V (row-major 3 x 3)
template <int P, int Q>
DICP_HD void nbl_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double* V) {
    if (apq == 0.0) return;
    const double diff = aqq - app;
    const double two = 2.0 * apq;
    const double zeta = diff / two;
    const double zz = zeta * zeta;
    const double h = 1.0 + zz;
    const double den = (zeta < 0.0 ? -zeta : zeta) + iss_sqrt(h);
    const double t = (zeta < 0.0 ? -1.0 : 1.0) / den;
    const double tt = t * t;
    const double g = 1.0 + tt;
    const double c = 1.0 / iss_sqrt(g);
    const double s = c * t;
    const double u = t * apq;
    app = app - u;
    aqq = aqq + u;
    apq = 0.0;
    const double cp = c * arp;
    const double sq = s * arq;
    const double sp = s * arp;
    const double cq = c * arq;
    arp = cp - sq;
    arq = sp + cq;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double vp = V[3 * r + P], vq = V[3 * r + Q];
        const double cvp = c * vp;
        const double svq = s * vq;
        const double svp = s * vp;
        const double cvq = c * vq;
        V[3 * r + P] = cvp - svq;
        V[3 * r + Q] = svp + cvq;
    }
}
DICP_HD double nbl_pick(int i, double a, double b, double c) { return i == 0 ? a : (i == 1 ? b : c); }
DICP_HD void nbl_exchange(double& lo, int& ilo, double& hi, int& ihi) {
    if (lo > hi) { const double t = lo; lo = hi; hi = t; const int i = ilo; ilo = ihi; ihi = i; }
}
// the eigen-system of the symmetric a = (xx, xy, xz, yy, yz, zz); a is overwritten.  -> lam ascending, v = [v_0 | v_1 | v_2] as three
// rows of 3 (nrm_grad_cov's layout)
DICP_HD void nbl_eigen(double* a, double* lam, double* v, int sweeps = ISS_SWEEPS) {
    double V[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    for (int it = 0; it < sweeps; ++it) {
        if (a[1] == 0.0 && a[2] == 0.0 && a[4] == 0.0) break;      // (every rotation left would be skipped)
        nbl_rotate<0, 1>(a[0], a[3], a[1], a[2], a[4], V);
        nbl_rotate<0, 2>(a[0], a[5], a[2], a[1], a[4], V);
        nbl_rotate<1, 2>(a[3], a[5], a[4], a[1], a[2], V);
    }
    int i0 = 0, i1 = 1, i2 = 2;
    lam[0] = a[0]; lam[1] = a[3]; lam[2] = a[5];
    nbl_exchange(lam[0], i0, lam[1], i1);                           // (a bubble sort with a strict compare: ties keep the lower index first)
    nbl_exchange(lam[1], i1, lam[2], i2);
    nbl_exchange(lam[0], i0, lam[1], i1);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        v[r] = nbl_pick(i0, V[3 * r], V[3 * r + 1], V[3 * r + 2]);
        v[3 + r] = nbl_pick(i1, V[3 * r], V[3 * r + 1], V[3 * r + 2]);
        v[6 + r] = nbl_pick(i2, V[3 * r], V[3 * r + 1], V[3 * r + 2]);
    }
}

// nrm_sign's rule with the dot product at statement level
DICP_HD double nbl_sign(const double* v0, const double* d) {
    const double x = v0[0] * d[0];
    const double y = v0[1] * d[1];
    const double z = v0[2] * d[2];
    const double xy = x + y;
    const double dot = xy + z;
    if (dot > 0) return 1.0;
    if (dot < 0) return -1.0;
    const double f = v0[0] != 0 ? v0[0] : (v0[1] != 0 ? v0[1] : v0[2]);
    return f < 0 ? -1.0 : 1.0;
}
DICP_HD double nbl_curvature(const double* lam) {
    const double a = lam[0] + lam[1];
    const double t = a + lam[2];
    return t > 0 ? lam[0] / t : 0.0;
}

// The forward of the live row in sorted slot s: row(j) the packed row of slot j (.x .y .z of T), vp the viewpoint.  -> lam[3], nrm[3],
// curvature, state[NBL_STATE] (doubles, not yet rounded); the count and the slots visited by the two walks through the references.
template <typename T, typename Keys, typename Row>
DICP_HD void nbl_forward_row(const BallPlan<T>& P, T R, double radius2, int s, const Keys& keys, const Row& row, const double* vp,
                             int min_neighbors, double* lam, double* nrm, double& curvature, double* state, int& count, unsigned& visited) {
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
#pragma unroll
    for (int e = 0; e < 6; ++e) state[NBL_C + e] = a[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) state[NBL_MU + e] = mu[e];
    state[NBL_N] = (double)n;
    double v[9];
    nbl_eigen(a, lam, v);
    const double d[3] = {vp[0] - pi[0], vp[1] - pi[1], vp[2] - pi[2]};
    const double sg = nbl_sign(v, d);
    const bool on = n >= min_neighbors;
    state[NBL_S] = on ? sg : 0.0;
#pragma unroll
    for (int e = 0; e < 3; ++e) nrm[e] = on ? sg * v[e] : 0.0;
    curvature = on ? nbl_curvature(lam) : 0.0;
    count = n;
}

// The record of a row from its state: p the row's coordinates, gn (3) / gk the cotangents of its normal and curvature (has_gn / has_gk
// false: absent, the value is not examined).  live false (a row outside the grid): state is not read.
DICP_HD void nbl_record(bool live, const double* state, const double* p, bool has_gn, const double* gn, bool has_gk, double gk, double tau,
                        double* Rec) {
    double G6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, mu[3] = {0.0, 0.0, 0.0};
    bool on = live && state[NBL_S] != 0.0;
    const bool any_gn = has_gn && (gn[0] != 0.0 || gn[1] != 0.0 || gn[2] != 0.0);   // (a NaN cotangent is not zero)
    const bool any_gk = has_gk && gk != 0.0;
    on = on && (any_gn || any_gk);
    int n = 1;
    if (on) {
        double a[6], lam[3], v[9];
#pragma unroll
        for (int e = 0; e < 6; ++e) a[e] = state[NBL_C + e];
#pragma unroll
        for (int e = 0; e < 3; ++e) mu[e] = state[NBL_MU + e];
        n = (int)state[NBL_N];
        nbl_eigen(a, lam, v);                               // (the forward's statements on the forward's C: the same lam and v)
        if (any_gn) on = nrm_grad_cov(lam, v, state[NBL_S], gn, any_gk ? gk : 0.0, tau, G6);       // (two calls: gn stays in registers)
        else on = nrm_grad_cov(lam, v, state[NBL_S], nullptr, gk, tau, G6);
    }
    nrm_det_record(Rec, on, G6, mu, p, n);
}

// the three terms of one member: Rec the member's record, y the receiving row's coordinates (nrm_det_term without the rounding to T)
DICP_HD void nbl_term(const double* Rec, const double* y, double* t) {
    double d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double e = y[c] - Rec[NRM_REC_P + c];
        d[c] = e - Rec[NRM_REC_MU + c];
    }
    const double* G = Rec + NRM_REC_G;
    const double g[3][3] = {{G[0], G[1], G[2]}, {G[1], G[3], G[4]}, {G[2], G[4], G[5]}};
    const double f = Rec[NRM_REC_F];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double p0 = g[a][0] * d[0];
        const double p1 = g[a][1] * d[1];
        const double s1 = p0 + p1;
        const double p2 = g[a][2] * d[2];
        const double s2 = s1 + p2;
        t[a] = f * s2;
    }
}
DICP_HD void nbl_gather_add(const double* Rec, const double* y, double* g) {
    if (Rec[NRM_REC_F] == 0.0) return;
    double t[3];
    nbl_term(Rec, y, t);
    g[0] = g[0] + t[0];
    g[1] = g[1] + t[1];
    g[2] = g[2] + t[2];
}

// The gradient of the live row in sorted slot s: rec(j) the record of slot j (const double*).  -> g[3] in double (rounded once to T by
// the caller) and the slots visited by the one walk.
template <typename T, typename Keys, typename Row, typename Rec>
DICP_HD void nbl_gather_row(const BallPlan<T>& P, T R, double radius2, int s, const Keys& keys, const Row& row, const Rec& rec, double* g,
                            unsigned& visited) {
    const auto self = row(s);
    double pj[3];
    iss_ball_load(self, pj);
    g[0] = 0.0; g[1] = 0.0; g[2] = 0.0;
    nbl_gather_add(rec(s), pj, g);                          // the row itself first
    visited = iss_ball_scan<T>(P, R, (T)self.x, (T)self.y, (T)self.z, keys, [&](int i) {
        if (i == s) return false;
        double pi[3], q[3];
        iss_ball_load(row(i), pi);
        const double r2 = iss_d2(pj, pi, q);
        if (iss_member(true, r2, radius2)) nbl_gather_add(rec(i), pj, g);
        return false;
    });
}

}  // namespace dicp
