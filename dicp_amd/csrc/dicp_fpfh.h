// The rules of the FPFH descriptor (dicp_amd/fpfh.py, csrc/fpfh.hip): Fast Point Feature Histograms (Rusu, Blodow, Beetz 2009), 33 channels,
// from points, normals and a (m, k) SELF neighbour index with -1 in empty slots.
//
// Plain inline C++, included by the HIP kernels and by a TEST-ONLY g++ build (tests/test_fpfh_host.py) that holds these rules to
// numpy (tests/fpfh_ref.py): the bin counts integer for integer, the descriptor bit for bit, on a CPU box with no GPU.
//
// Everything is in double; float inputs are converted exactly.  The only operations are + - * / sqrt and comparisons: no fma, no libm.
// The build contracts a * b + c only inside ONE expression (-ffp-contract=on): every product that is added to something is a statement of
// its own below.
//
// Row i is OK when its three coordinates and three normal components are finite and the normal is not (0, 0, 0).
// Slot (i, s) with j = idx[i, s] is NEAR when i < rows, 0 <= j < rows (one unsigned compare, dicp_group.h), j != i, both rows are OK,
//   r2 = (dx dx + dy dy) + dz dz > 0 with d = p_j - p_i and every product rounded, and r2 <= radius2 when a radius was given.
// A near slot is a PAIR when its Darboux frame exists (Open3D's ComputePairFeatures):
//   r = sqrt(r2); a1 = (n_i . d) / r; a2 = (n_j . d) / r
//   |a1| < |a2|: n1 = n_j, n2 = n_i, d = -d, phi = -a2; otherwise (a tie included) n1 = n_i, n2 = n_j, phi = a1
//   v = d x n1; q = v . v; no frame unless q > 0; v = v / sqrt(q); w = n1 x v
//   sin = w . n2; cos = n1 . n2; alpha = v . n2
//   every dot product is (x + y) + z over the rounded products; a cross product's component is the difference of two rounded products,
//   (a x b)_0 = a1 b2 - a2 b1, (a x b)_1 = a2 b0 - a0 b2, (a x b)_2 = a0 b1 - a1 b0.
// Bins, eleven per feature: alpha and phi take clamp(floor(11 ((a + 1) 0.5)), 0, 10) (a NaN: 0).  theta, the angle of (cos, sin) in
//   (-pi, pi], takes the number of edges beta_t = -pi + 2 pi t / 11 (t = 1 .. 10) at or below it, decided without atan2 by half-plane tests
//   against the table below: with cr = cos(beta) sin - sin(beta) cos, an edge of the lower half plane counts when sin >= 0 or cr >= 0, an
//   edge of the upper one when sin >= 0 and cr >= 0.
// SPFH: cnt[i, 0:11 | 11:22 | 22:33] are the theta | alpha | phi bin counts over the pairs of row i, c_i their number;
//   s_i[ch] = (100 cnt[i, ch]) / c_i, 0 when c_i = 0.
// FPFH: over the NEAR slots of row i (a frame is not asked for) in slot order from +0: wj = 1 / r2, t = wj s_j[ch], acc[ch] = acc[ch] + t;
//   per group of 11 channels S = the sum of acc in ascending channel order from +0; out[ch] = (S != 0 ? acc[ch] (100 / S) : 0) + s_i[ch],
//   rounded once to the points' type.  A row that is not OK, or at or past `rows`, has no near slot and gets 33 zeros.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dicp_group.h"
#include "dicp_math.h"

namespace dicp {

constexpr int FPFH_BINS = 11, FPFH_CH = 33;
constexpr int FPFH_K_MIN = 1, FPFH_K_MAX = 32;
// A row of the internal SPFH table: bytes 0:33 the counts (each <= k <= 32), byte 33 c_i, byte 34 the row's OK flag, the rest 0.
// 48 bytes: three aligned 16-byte words per gathered neighbour.
constexpr int FPFH_ROW_BYTES = 48, FPFH_ROW_C = 33, FPFH_ROW_OK = 34;

// IEEE square root: correctly rounded on the host and in the device library (the GPU tests compare bit for bit with numpy's).
DICP_HD double fpfh_sqrt(double x) { return sqrt(x); }

DICP_HD bool fpfh_finite(double x) { return x - x == 0.0; }
DICP_HD bool fpfh_row_ok(const double* p, const double* n) {
    return fpfh_finite(p[0]) && fpfh_finite(p[1]) && fpfh_finite(p[2]) && fpfh_finite(n[0]) && fpfh_finite(n[1]) && fpfh_finite(n[2])
           && (n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0);
}

// the row a slot of row i names, or -1: empty, out of range, or i itself
DICP_HD int fpfh_neighbour(int64_t j, int i, int rows) { const int r = group_row(j, rows); return r == i ? -1 : r; }
DICP_HD int fpfh_neighbour(int32_t j, int i, int rows) { const int r = group_row(j, rows); return r == i ? -1 : r; }

DICP_HD double fpfh_dot(const double* a, const double* b) {
    const double x = a[0] * b[0];
    const double y = a[1] * b[1];
    const double z = a[2] * b[2];
    const double s = x + y;
    return s + z;
}
DICP_HD void fpfh_cross(const double* a, const double* b, double* c) {
    const double t0 = a[1] * b[2];
    const double u0 = a[2] * b[1];
    const double t1 = a[2] * b[0];
    const double u1 = a[0] * b[2];
    const double t2 = a[0] * b[1];
    const double u2 = a[1] * b[0];
    c[0] = t0 - u0;
    c[1] = t1 - u1;
    c[2] = t2 - u2;
}

// d = pj - pi -> r2
DICP_HD double fpfh_d2(const double* pi, const double* pj, double* d) {
    d[0] = pj[0] - pi[0];
    d[1] = pj[1] - pi[1];
    d[2] = pj[2] - pi[2];
    return fpfh_dot(d, d);
}
// the near test of a slot whose index names a live row other than i.  radius2 < 0: no radius
DICP_HD bool fpfh_near(bool ok_i, bool ok_j, double r2, double radius2) {
    return ok_i && ok_j && r2 > 0.0 && (radius2 < 0.0 || r2 <= radius2);
}

// the bin of alpha or phi
DICP_HD int fpfh_bin_unit(double a) {
    const double h = a + 1.0;
    const double u = h * 0.5;
    const double x = 11.0 * u;
    if (!(x >= 1.0)) return 0;              // (a NaN too)
    if (x >= 10.0) return 10;
    return (int)x;                          // 1 <= x < 10: truncation is the floor
}

// 1 when the edge (cb, sb) = (cos beta, sin beta) lies at or below the angle of (c, s)
DICP_HD int fpfh_edge(double cb, double sb, double c, double s) {
    const double t = cb * s;
    const double u = sb * c;
    const double cr = t - u;
    return sb < 0.0 ? ((s >= 0.0 || cr >= 0.0) ? 1 : 0) : ((s >= 0.0 && cr >= 0.0) ? 1 : 0);
}
// the bin of theta: (cos beta_t, sin beta_t) of beta_t = -pi + 2 pi t / 11, t = 1 .. 10, as double literals
DICP_HD int fpfh_bin_theta(double c, double s) {
    int b = 0;
    b += fpfh_edge(-0.8412535328311811, -0.5406408174555978, c, s);
    b += fpfh_edge(-0.4154150130018863, -0.9096319953545184, c, s);
    b += fpfh_edge(0.14231483827328512, -0.9898214418809327, c, s);
    b += fpfh_edge(0.6548607339452851, -0.7557495743542583, c, s);
    b += fpfh_edge(0.9594929736144975, -0.2817325568414295, c, s);
    b += fpfh_edge(0.9594929736144975, 0.2817325568414295, c, s);
    b += fpfh_edge(0.6548607339452851, 0.7557495743542583, c, s);
    b += fpfh_edge(0.14231483827328512, 0.9898214418809327, c, s);
    b += fpfh_edge(-0.41541501300188616, 0.9096319953545186, c, s);
    b += fpfh_edge(-0.8412535328311813, 0.5406408174555974, c, s);
    return b;
}

DICP_HD double fpfh_abs(double x) { return x < 0.0 ? -x : x; }

// The three features of a near slot -> false when there is no frame.  d (= pj - pi) is overwritten.
DICP_HD bool fpfh_pair_features(const double* ni, const double* nj, double* d, double r2, double* cos_t, double* sin_t, double* alpha, double* phi) {
    const double r = fpfh_sqrt(r2);
    const double a1 = fpfh_dot(ni, d) / r;
    const double a2 = fpfh_dot(nj, d) / r;
    const bool swap = fpfh_abs(a1) < fpfh_abs(a2);      // (selects, not pointers: the kernels keep all of this in registers)
    double n1[3], n2[3], v[3], w[3];
    for (int a = 0; a < 3; ++a) {
        n1[a] = swap ? nj[a] : ni[a];
        n2[a] = swap ? ni[a] : nj[a];
        d[a] = swap ? -d[a] : d[a];
    }
    *phi = swap ? -a2 : a1;
    fpfh_cross(d, n1, v);
    const double q = fpfh_dot(v, v);
    if (!(q > 0.0)) return false;
    const double sq = fpfh_sqrt(q);
    v[0] = v[0] / sq; v[1] = v[1] / sq; v[2] = v[2] / sq;
    fpfh_cross(n1, v, w);
    *sin_t = fpfh_dot(w, n2);
    *cos_t = fpfh_dot(n1, n2);
    *alpha = fpfh_dot(v, n2);
    return true;
}
// -> the three channels (theta, 11 + alpha, 22 + phi) of a near slot, false when it is no pair
DICP_HD bool fpfh_pair_bins(const double* ni, const double* nj, double* d, double r2, int* ch) {
    double c, s, a, f;
    if (!fpfh_pair_features(ni, nj, d, r2, &c, &s, &a, &f)) return false;
    ch[0] = fpfh_bin_theta(c, s);
    ch[1] = FPFH_BINS + fpfh_bin_unit(a);
    ch[2] = 2 * FPFH_BINS + fpfh_bin_unit(f);
    return true;
}

// s_i[ch] from a count and the row's number of pairs
DICP_HD double fpfh_spfh(int cnt, int c) {
    const double h = 100.0 * (double)cnt;
    return c > 0 ? h / (double)c : 0.0;
}
DICP_HD double fpfh_weight(double r2) { return 1.0 / r2; }
DICP_HD double fpfh_weight_add(double acc, double wj, double s) {
    const double t = wj * s;
    return acc + t;
}
DICP_HD double fpfh_out(double acc, double S, double s_i) {
    double u = 0.0;
    if (S != 0.0) {
        const double f = 100.0 / S;
        u = acc * f;
    }
    return u + s_i;
}

}  // namespace dicp
