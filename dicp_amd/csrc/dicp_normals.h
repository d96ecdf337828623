// Per-point arithmetic of the surface-normal estimate (dicp_amd/normals.py, csrc/normals.hip).
//
// Plain inline C++ on doubles, included by the HIP kernels and by a TEST-ONLY g++ build (tests/test_normals_host.py)
// that checks these formulas against numpy / torch autograd on a CPU box with no GPU.
//
// For a point p_i with k_eff >= 3 neighbours p_j (itself among them):
//   q_j = p_j - p_i;  mu = mean q;  C = (1/k_eff) sum (q_j - mu)(q_j - mu)^T           (two passes over the neighbours)
//   C = sum lam_a v_a v_a^T, lam_0 <= lam_1 <= lam_2 (svd3 of the symmetric C);  n = s v_0,  s = +-1 so that n . (viewpoint - p_i) >= 0
//   curvature = lam_0 / (lam_0 + lam_1 + lam_2), 0 when the trace is 0.
// Backward, with gn = dL/dn and gk = dL/dcurvature:
//   M = sum_{a=1,2} (s gn . v_a) / (lam_0 - lam_a) v_a v_0^T  +  gk ((1/T) v_0 v_0^T - (lam_0/T^2) I);   G = (M + M^T) / 2
//   dL/dp_j = (2/k_eff) G (q_j - mu) for every neighbour j (q_j - mu does not depend on p_i: the mean removes it).
// A point whose two smallest eigenvalues are not separated (lam_1 - lam_0 <= tau T) contributes G = 0: its v_0 is not a function
// of the points there, and 1/(lam_0 - lam_1) would be inf or NaN.
#pragma once
#include "dicp_math.h"

namespace dicp {

// C6 = [xx, xy, xz, yy, yz, zz]: one neighbour's (q_j - mu) outer product added
DICP_HD void nrm_cov_add(double* C6, const double* d) {
    C6[0] += d[0] * d[0]; C6[1] += d[0] * d[1]; C6[2] += d[0] * d[2];
    C6[3] += d[1] * d[1]; C6[4] += d[1] * d[2]; C6[5] += d[2] * d[2];
}

// Eigen-decomposition of the symmetric PSD C6 through svd3: lam ascending, v = [v_0 | v_1 | v_2] as three rows of 3.
// svd3's V is orthogonal by construction (a product of rotations) and its singular values of a PSD matrix are its eigenvalues.
DICP_HD void nrm_eig(const double* C6, double* lam, double* v) {
    const double A[9] = {C6[0], C6[1], C6[2], C6[1], C6[3], C6[4], C6[2], C6[4], C6[5]};
    double U[9], S[3], V[9];
    svd3(A, U, S, V);
    lam[0] = S[2]; lam[1] = S[1]; lam[2] = S[0];
    v[0] = V[2]; v[1] = V[5]; v[2] = V[8];          // smallest singular value: column 2
    v[3] = V[1]; v[4] = V[4]; v[5] = V[7];
    v[6] = V[0]; v[7] = V[3]; v[8] = V[6];
}

// The sign s that makes s v0 . d >= 0, d = viewpoint - p_i; on a dot product of exactly 0, the one that makes v0's first nonzero component positive
DICP_HD double nrm_sign(const double* v0, const double* d) {
    const double dot = v0[0] * d[0] + v0[1] * d[1] + v0[2] * d[2];
    if (dot > 0) return 1.0;
    if (dot < 0) return -1.0;
    const double f = v0[0] != 0 ? v0[0] : (v0[1] != 0 ? v0[1] : v0[2]);
    return f < 0 ? -1.0 : 1.0;
}

DICP_HD double nrm_curvature(const double* lam) {
    const double T = lam[0] + lam[1] + lam[2];
    return T > 0 ? lam[0] / T : 0.0;
}

// G6 (same layout as C6) = dL/dC, symmetrised; returns false (and G6 = 0) where the point contributes no gradient
DICP_HD bool nrm_grad_cov(const double* lam, const double* v, double s, const double* gn, double gk, double tau, double* G6) {
    for (int e = 0; e < 6; ++e) G6[e] = 0.0;
    const double T = lam[0] + lam[1] + lam[2];
    if (!(T > 0) || !(lam[1] - lam[0] > tau * T)) return false;
    const double* v0 = v;
    double M[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) M[e] = 0.0;
    if (gn) {
#pragma unroll
        for (int a = 1; a < 3; ++a) {
            const double* va = v + 3 * a;
            const double w = s * (gn[0] * va[0] + gn[1] * va[1] + gn[2] * va[2]) / (lam[0] - lam[a]);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) M[r * 3 + c] += w * va[r] * v0[c];
        }
    }
    if (gk != 0.0) {
        const double a = gk / T, b = gk * lam[0] / (T * T);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) M[r * 3 + c] += a * v0[r] * v0[c] - (r == c ? b : 0.0);
    }
    G6[0] = M[0]; G6[3] = M[4]; G6[5] = M[8];
    G6[1] = 0.5 * (M[1] + M[3]); G6[2] = 0.5 * (M[2] + M[6]); G6[4] = 0.5 * (M[5] + M[7]);
    return true;
}

// dL/dp_j = (2/k_eff) G (q_j - mu)
DICP_HD void nrm_point_grad(const double* G6, const double* d, int k_eff, double* g) {
    const double f = 2.0 / k_eff;
    g[0] = f * (G6[0] * d[0] + G6[1] * d[1] + G6[2] * d[2]);
    g[1] = f * (G6[1] * d[0] + G6[3] * d[1] + G6[4] * d[2]);
    g[2] = f * (G6[2] * d[0] + G6[4] * d[1] + G6[5] * d[2]);
}

}  // namespace dicp
