// The rules of the ISS keypoint detector (dicp_amd/iss.py, csrc/iss.hip): Intrinsic Shape Signatures (Zhong 2009) in the form of Open3D's
// ComputeISSKeypoints, from points and a (m, k) SELF neighbour index with -1 in empty slots.
//
// Plain inline C++, included by the HIP kernels and by a TEST-ONLY g++ build (tests/test_iss_host.py) that holds these rules to numpy
// (tests/iss_ref.py): eigenvalues, saliency and counts bit for bit, the keypoint mask exactly, on a CPU box with no GPU.
//
// Everything is in double; float inputs are converted exactly.  The only operations are + - * / sqrt and comparisons: no fma, no libm.
// The build contracts a * b + c only inside ONE expression (-ffp-contract=on): every product that is added to something is a statement of
// its own below.
//
// Row i is OK when its three coordinates are finite.
// Slot (i, s) with j = idx[i, s] is LIVE when 0 <= j < rows (one unsigned compare, dicp_group.h) and j != i: the row itself is skipped
//   wherever it stands.
// MEMBERS of row i for a radius R (radius2 = R R; radius2 < 0: no cut): row i itself first, then, in slot order, the live slots whose row is
//   OK and whose r2 = (dx dx + dy dy) + dz dz <= radius2 with d = p_j - p_i and every product rounded.  Duplicates (r2 = 0) ARE members;
//   a row named by two slots is a member twice.  count_i is their number, the row itself included.
// Covariance, on q_j = p_j - p_i (q_i = 0): mu = (the sum of q over the members in that order from +0) / count; d = q - mu; the six sums
//   xx, xy, xz, yy, yz, zz of the rounded products d_a d_b in member order from +0, each divided by count.
// Eigenvalues: two-sided cyclic Jacobi on the six entries, pairs in the order (0,1), (0,2), (1,2), exactly ISS_SWEEPS sweeps.  A rotation
//   whose a_pq is exactly 0 is skipped.  Otherwise
//     zeta = (a_qq - a_pp) / (2 a_pq);  t = sign(zeta) / (|zeta| + sqrt(1 + zeta zeta)), sign(0) = +1;  c = 1 / sqrt(1 + t t);  s = c t
//     a_pp -= t a_pq;  a_qq += t a_pq;  a_pq = 0;  for the third index r: (a_rp, a_rq) <- (c a_rp - s a_rq, s a_rp + c a_rq)
//   then l0 <= l1 <= l2 by three compare-exchanges.  No eigenvectors.
//   ISS_SWEEPS = 6: tests/test_iss_host.py runs the statement-level restatement over uniform, planar (1e-3) and linear (1e-4)
//   neighbourhoods, clouds 2.5 km from the origin and count = 3, and finds every off-diagonal exactly 0 after at most 6 sweeps (the
//   largest number any of them needed is recorded in profiles/r31_iss_edges.txt).  Six is kept for those exact zeros only: the three
//   eigenvalues stop changing after the fourth sweep on every matrix sampled there, so a fifth or sixth sweep shows in no output, and
//   the early exit of iss_eigenvalues (every off-diagonal already 0: all rotations left would be skipped) makes them cost nothing
//   where they are not needed.  Do not read the constant as an accuracy knob.
// Saliency (Open3D's rule, with products instead of quotients: nothing divides by 0): sal_i = l0 when
//   count_i >= min_neighbors, l1 < gamma21 l2 and 0 < l0 < gamma32 l1; otherwise 0.  A row that is not OK, or at or past `rows`, gets 0
//   (and eigenvalues 0, count 0).
// Keypoint (non-maximum suppression over a second member set with its own radius): sal_i > 0, the member count for that radius is at
//   least min_neighbors, and no member j has sal_j > sal_i, or sal_j == sal_i and j < i.  The tie rule is the one departure from Open3D,
//   which keeps both sides of an exact tie: exact duplicates yield one keypoint.  The comparison is on the DOUBLE saliencies.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dicp_group.h"
#include "dicp_math.h"

namespace dicp {

constexpr int ISS_SWEEPS = 6;
constexpr int ISS_K_MIN = 1, ISS_K_MAX = 32;

// IEEE square root: correctly rounded on the host and in the device library (the GPU tests compare bit for bit with numpy's).
DICP_HD double iss_sqrt(double x) { return sqrt(x); }

DICP_HD bool iss_finite(double x) { return x - x == 0.0; }
DICP_HD bool iss_row_ok(const double* p) { return iss_finite(p[0]) && iss_finite(p[1]) && iss_finite(p[2]); }

// the row a slot of row i names, or -1: empty, out of range, or i itself
DICP_HD int iss_neighbour(int64_t j, int i, int rows) { const int r = group_row(j, rows); return r == i ? -1 : r; }
DICP_HD int iss_neighbour(int32_t j, int i, int rows) { const int r = group_row(j, rows); return r == i ? -1 : r; }

// q = pj - pi -> r2
DICP_HD double iss_d2(const double* pi, const double* pj, double* q) {
    q[0] = pj[0] - pi[0];
    q[1] = pj[1] - pi[1];
    q[2] = pj[2] - pi[2];
    const double x = q[0] * q[0];
    const double y = q[1] * q[1];
    const double z = q[2] * q[2];
    const double s = x + y;
    return s + z;
}
// the member test of a live slot.  radius2 < 0: no radius
DICP_HD bool iss_member(bool ok_j, double r2, double radius2) { return ok_j && (radius2 < 0.0 || r2 <= radius2); }

// one member's q added to the running sum of the mean
DICP_HD void iss_mean_add(double* sum, const double* q) {
    sum[0] = sum[0] + q[0];
    sum[1] = sum[1] + q[1];
    sum[2] = sum[2] + q[2];
}
DICP_HD void iss_mean(const double* sum, int count, double* mu) {
    const double n = (double)count;
    mu[0] = sum[0] / n;
    mu[1] = sum[1] / n;
    mu[2] = sum[2] / n;
}
// one member's d = q - mu added to the six running sums a = (xx, xy, xz, yy, yz, zz)
DICP_HD void iss_cov_add(double* a, const double* q, const double* mu) {
    const double dx = q[0] - mu[0];
    const double dy = q[1] - mu[1];
    const double dz = q[2] - mu[2];
    const double xx = dx * dx;
    const double xy = dx * dy;
    const double xz = dx * dz;
    const double yy = dy * dy;
    const double yz = dy * dz;
    const double zz = dz * dz;
    a[0] = a[0] + xx;
    a[1] = a[1] + xy;
    a[2] = a[2] + xz;
    a[3] = a[3] + yy;
    a[4] = a[4] + yz;
    a[5] = a[5] + zz;
}
DICP_HD void iss_cov_scale(double* a, int count) {
    const double n = (double)count;
    a[0] = a[0] / n; a[1] = a[1] / n; a[2] = a[2] / n; a[3] = a[3] / n; a[4] = a[4] / n; a[5] = a[5] / n;
}

// one Jacobi rotation that annihilates apq; arp, arq: the entries that couple the third index r to p and to q
DICP_HD void iss_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
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
}
// one sweep over a = (a00, a01, a02, a11, a12, a22)
DICP_HD void iss_sweep(double* a) {
    iss_rotate(a[0], a[3], a[1], a[2], a[4]);       // (0,1): r = 2
    iss_rotate(a[0], a[5], a[2], a[1], a[4]);       // (0,2): r = 1
    iss_rotate(a[3], a[5], a[4], a[1], a[2]);       // (1,2): r = 0
}
DICP_HD void iss_exchange(double& lo, double& hi) {
    if (lo > hi) { const double t = lo; lo = hi; hi = t; }
}
// the eigenvalues of the symmetric a = (xx, xy, xz, yy, yz, zz), ascending; a is overwritten.  sweeps: ISS_SWEEPS (the tests pass others)
DICP_HD void iss_eigenvalues(double* a, double* l, int sweeps = ISS_SWEEPS) {
    for (int it = 0; it < sweeps; ++it) {
        if (a[1] == 0.0 && a[2] == 0.0 && a[4] == 0.0) break;      // (every rotation left would be skipped)
        iss_sweep(a);
    }
    l[0] = a[0]; l[1] = a[3]; l[2] = a[5];
    iss_exchange(l[0], l[1]);
    iss_exchange(l[1], l[2]);
    iss_exchange(l[0], l[1]);
}

DICP_HD double iss_saliency(const double* l, int count, double gamma21, double gamma32, int min_neighbors) {
    const double b21 = gamma21 * l[2];
    const double b32 = gamma32 * l[1];
    return (count >= min_neighbors && l[1] < b21 && 0.0 < l[0] && l[0] < b32) ? l[0] : 0.0;
}
// does member j suppress row i?
DICP_HD bool iss_beats(double sal_j, int j, double sal_i, int i) { return sal_j > sal_i || (sal_j == sal_i && j < i); }

}  // namespace dicp
