// TEST-ONLY host build of dicp_amd/csrc/dicp_normals.h (g++, no GPU): the per-point normal arithmetic the HIP kernels execute,
// driven the way csrc/normals.hip drives it (two passes over a neighbourhood), for tests/test_normals_host.py.  Never loaded by dicp_amd.
#include "../../dicp_amd/csrc/dicp_normals.h"

using namespace dicp;

// q (k,3): the neighbours' offsets p_j - p_i in the kernel's neighbour order; mu (3), C6 (6) out
static void cov(const double* q, int k, double* mu, double* C6) {
    double s[3] = {0, 0, 0};
    for (int o = 0; o < k; ++o) for (int a = 0; a < 3; ++a) s[a] += q[3 * o + a];
    for (int a = 0; a < 3; ++a) mu[a] = s[a] / k;
    for (int e = 0; e < 6; ++e) C6[e] = 0.0;
    for (int o = 0; o < k; ++o) {
        const double d[3] = {q[3 * o] - mu[0], q[3 * o + 1] - mu[1], q[3 * o + 2] - mu[2]};
        nrm_cov_add(C6, d);
    }
    for (int e = 0; e < 6; ++e) C6[e] /= k;
}

extern "C" {

// dv = viewpoint - p_i.  n (3), curvature (1), lam (3, ascending), v (9: v0 v1 v2 as rows)
void nc_forward(const double* q, int k, const double* dv, double* n, double* curv, double* lam, double* v) {
    double mu[3], C6[6];
    cov(q, k, mu, C6);
    nrm_eig(C6, lam, v);
    const double s = nrm_sign(v, dv);
    for (int a = 0; a < 3; ++a) n[a] = s * v[a];
    *curv = nrm_curvature(lam);
}

// gq (k,3): dL/dp_j for every neighbour; returns 1 where the point contributes, 0 where it does not
int nc_backward(const double* q, int k, const double* dv, const double* gn, double gk, double tau, double* gq) {
    double mu[3], C6[6], lam[3], v[9], G6[6];
    cov(q, k, mu, C6);
    nrm_eig(C6, lam, v);
    const double s = nrm_sign(v, dv);
    const bool on = nrm_grad_cov(lam, v, s, gn, gk, tau, G6);
    for (int o = 0; o < k; ++o) {
        const double d[3] = {q[3 * o] - mu[0], q[3 * o + 1] - mu[1], q[3 * o + 2] - mu[2]};
        nrm_point_grad(G6, d, k, gq + 3 * o);
    }
    return on ? 1 : 0;
}

}
