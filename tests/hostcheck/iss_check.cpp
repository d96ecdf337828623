// TEST-ONLY host build of dicp_amd/csrc/dicp_iss.h (g++, no GPU): the rules of the ISS keypoints that the HIP kernels execute, run in serial
// loops for tests/test_iss_host.py.  Never loaded by dicp_amd.
//
// variant 0 is the header's rule.  The others are WRONG rules, written out here, which the comparison with tests/iss_ref.py must refuse:
// 1 fewer Jacobi sweeps than ISS_SWEEPS (the caller says how many), 2 `<=` for `<` in the two gamma tests, 3 both sides of an exact tie
// stay keypoints, 4 a slot that names the row itself is not skipped (the row is counted twice), 5 the radius cut is dropped in the second
// pass.
#include <cstdint>
#include <vector>

#include "../../dicp_amd/csrc/dicp_iss.h"

using namespace dicp;

namespace {

enum { RIGHT = 0, FEW_SWEEPS = 1, GAMMA_LE = 2, TIE_BOTH = 3, SELF_TWICE = 4, NMS_NO_RADIUS = 5 };

template <typename T>
void load3(const T* p, double* v) { v[0] = (double)p[0]; v[1] = (double)p[1]; v[2] = (double)p[2]; }

template <typename I>
int neighbour(I j, int i, int rows, int variant) { return variant == SELF_TWICE ? group_row(j, rows) : iss_neighbour(j, i, rows); }

// variant 2: iss_saliency with `<=`
double saliency_le(const double* l, int count, double gamma21, double gamma32, int min_neighbors) {
    const double b21 = gamma21 * l[2];
    const double b32 = gamma32 * l[1];
    return (count >= min_neighbors && l[1] <= b21 && 0.0 < l[0] && l[0] <= b32) ? l[0] : 0.0;
}

// the two passes of csrc/iss.hip, one row and one slot after the other
template <typename T, typename I>
void cloud(const T* pts, int c, const I* idx, int k, const I* nms, int k2, int m, int rows, double r1, double r2, double g21, double g32, int min_nb,
           int variant, int sweeps, T* eig, T* sal_out, int32_t* cnt, uint8_t* mask) {
    const double rad1 = r1 == 0.0 ? -1.0 : r1 * r1;
    const double rad2 = (r2 == 0.0 || variant == NMS_NO_RADIUS) ? -1.0 : r2 * r2;
    std::vector<double> sal((size_t)m, 0.0);
    for (int i = 0; i < m; ++i) {
        double pi[3] = {0.0, 0.0, 0.0}, l[3] = {0.0, 0.0, 0.0};
        int count = 0;
        bool ok_i = false;
        if (i < rows) {
            load3(pts + (size_t)i * c, pi);
            ok_i = iss_row_ok(pi);
        }
        if (ok_i) {
            double sum[3] = {0.0, 0.0, 0.0};
            uint32_t members = 0u;
            count = 1;
            for (int s = 0; s < k; ++s) {
                const int j = neighbour(idx[(size_t)i * k + s], i, rows, variant);
                if (j < 0) continue;
                double pj[3], q[3];
                load3(pts + (size_t)j * c, pj);
                const double d2 = iss_d2(pi, pj, q);
                if (!iss_member(iss_row_ok(pj), d2, rad1)) continue;
                members |= 1u << s;
                ++count;
                iss_mean_add(sum, q);
            }
            double mu[3], a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            const double zero[3] = {0.0, 0.0, 0.0};
            iss_mean(sum, count, mu);
            iss_cov_add(a, zero, mu);
            for (int s = 0; s < k; ++s) {
                if (!((members >> s) & 1u)) continue;
                const int j = neighbour(idx[(size_t)i * k + s], i, rows, variant);
                double pj[3], q[3];
                load3(pts + (size_t)j * c, pj);
                iss_d2(pi, pj, q);
                iss_cov_add(a, q, mu);
            }
            iss_cov_scale(a, count);
            iss_eigenvalues(a, l, variant == FEW_SWEEPS ? sweeps : ISS_SWEEPS);
            sal[(size_t)i] = variant == GAMMA_LE ? saliency_le(l, count, g21, g32, min_nb) : iss_saliency(l, count, g21, g32, min_nb);
        }
        sal_out[i] = (T)sal[(size_t)i];
        for (int a = 0; a < 3; ++a) eig[(size_t)i * 3 + a] = (T)l[a];
        cnt[i] = count;
    }
    for (int i = 0; i < m; ++i) {
        const double sal_i = sal[(size_t)i];
        bool keep = i < rows && sal_i > 0.0;
        if (keep) {
            double pi[3];
            load3(pts + (size_t)i * c, pi);
            int count = 1;
            for (int s = 0; s < k2; ++s) {
                const int j = iss_neighbour(nms[(size_t)i * k2 + s], i, rows);
                if (j < 0) continue;
                double pj[3], q[3];
                load3(pts + (size_t)j * c, pj);
                const double d2 = iss_d2(pi, pj, q);
                if (!iss_member(iss_row_ok(pj), d2, rad2)) continue;
                ++count;
                const double sal_j = sal[(size_t)j];
                if (variant == TIE_BOTH ? sal_j > sal_i : iss_beats(sal_j, j, sal_i, i)) keep = false;
            }
            keep = keep && count >= min_nb;
        }
        mask[i] = keep ? 1 : 0;
    }
}

template <typename T>
void cloud_i(int idx64, const void* pts, int c, const void* idx, int k, const void* nms, int k2, int m, int rows, double r1, double r2, double g21,
             double g32, int min_nb, int variant, int sweeps, void* eig, void* sal, int32_t* cnt, uint8_t* mask) {
    if (idx64) cloud<T, int64_t>((const T*)pts, c, (const int64_t*)idx, k, (const int64_t*)nms, k2, m, rows, r1, r2, g21, g32, min_nb, variant, sweeps, (T*)eig, (T*)sal, cnt, mask);
    else cloud<T, int32_t>((const T*)pts, c, (const int32_t*)idx, k, (const int32_t*)nms, k2, m, rows, r1, r2, g21, g32, min_nb, variant, sweeps, (T*)eig, (T*)sal, cnt, mask);
}

}  // namespace

extern "C" {

// ISS_SWEEPS, ISS_K_MIN, ISS_K_MAX
void isc_constants(int32_t* out) { out[0] = ISS_SWEEPS; out[1] = ISS_K_MIN; out[2] = ISS_K_MAX; }

// the eigenvalues of n symmetric matrices a (n, 6) = (xx, xy, xz, yy, yz, zz) after `sweeps` sweeps -> lam (n, 3) ascending, and the six
// entries as the sweeps left them -> worked (n, 6)
void isc_eigenvalues(const double* a, int n, int sweeps, double* lam, double* worked) {
    for (int i = 0; i < n; ++i) {
        double* w = worked + (size_t)i * 6;
        for (int e = 0; e < 6; ++e) w[e] = a[(size_t)i * 6 + e];
        iss_eigenvalues(w, lam + (size_t)i * 3, sweeps);
    }
}

// one cloud, both passes.  idx (m, k) for the saliency, nms (m, k2) for the suppression; a radius of 0: none; sweeps: read by variant 1.
void isc_cloud(int f64, int idx64, const void* pts, int c, const void* idx, int k, const void* nms, int k2, int m, int rows, double r1, double r2,
               double g21, double g32, int min_nb, int variant, int sweeps, void* eig, void* sal, int32_t* cnt, uint8_t* mask) {
    if (f64) cloud_i<double>(idx64, pts, c, idx, k, nms, k2, m, rows, r1, r2, g21, g32, min_nb, variant, sweeps, eig, sal, cnt, mask);
    else cloud_i<float>(idx64, pts, c, idx, k, nms, k2, m, rows, r1, r2, g21, g32, min_nb, variant, sweeps, eig, sal, cnt, mask);
}

}
