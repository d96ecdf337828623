// TEST-ONLY host build of dicp_amd/csrc/dicp_fpfh.h (g++, no GPU): the rules of the FPFH descriptor that the HIP kernels execute, run in
// serial loops for tests/test_fpfh_host.py.  Never loaded by dicp_amd.
//
// variant 0 is the header's rule.  The others are WRONG rules, written out here, which the comparison with tests/fpfh_ref.py must refuse:
// 1 the roles swap on a tie |a1| = |a2| too, 2 `>` for `>=` in the sine test of a lower-half-plane edge, 3 the row itself (and any slot at
// distance 0) stays among its neighbours, 4 the weight is 1 / the search's d2 instead of the recomputed one, 5 the counts are divided by k
// instead of the number of pairs.
#include <cstdint>
#include <vector>

#include "../../dicp_amd/csrc/dicp_fpfh.h"

using namespace dicp;

namespace {

enum { RIGHT = 0, TIE_SWAP = 1, STRICT_EDGE = 2, KEEP_SELF = 3, SEARCH_D2 = 4, NORM_K = 5 };

// variant 1: fpfh_pair_features with `<=`
bool features_tie_swap(const double* ni, const double* nj, double* d, double r2, double* cos_t, double* sin_t, double* alpha, double* phi) {
    const double r = fpfh_sqrt(r2);
    const double a1 = fpfh_dot(ni, d) / r;
    const double a2 = fpfh_dot(nj, d) / r;
    const bool swap = fpfh_abs(a1) <= fpfh_abs(a2);
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

// variant 2: the lower-half-plane edges (t = 1 .. 5) ask sin > 0
int edge_strict(double cb, double sb, double c, double s) {
    const double t = cb * s;
    const double u = sb * c;
    const double cr = t - u;
    return (s > 0.0 || cr >= 0.0) ? 1 : 0;
}
int theta_strict(double c, double s) {
    int b = 0;
    b += edge_strict(-0.8412535328311811, -0.5406408174555978, c, s);
    b += edge_strict(-0.4154150130018863, -0.9096319953545184, c, s);
    b += edge_strict(0.14231483827328512, -0.9898214418809327, c, s);
    b += edge_strict(0.6548607339452851, -0.7557495743542583, c, s);
    b += edge_strict(0.9594929736144975, -0.2817325568414295, c, s);
    b += fpfh_edge(0.9594929736144975, 0.2817325568414295, c, s);
    b += fpfh_edge(0.6548607339452851, 0.7557495743542583, c, s);
    b += fpfh_edge(0.14231483827328512, 0.9898214418809327, c, s);
    b += fpfh_edge(-0.41541501300188616, 0.9096319953545186, c, s);
    b += fpfh_edge(-0.8412535328311813, 0.5406408174555974, c, s);
    return b;
}

bool pair_bins(const double* ni, const double* nj, double* d, double r2, int variant, int* ch) {
    if (variant != TIE_SWAP && variant != STRICT_EDGE) return fpfh_pair_bins(ni, nj, d, r2, ch);
    double c, s, a, f;
    const bool frame = variant == TIE_SWAP ? features_tie_swap(ni, nj, d, r2, &c, &s, &a, &f) : fpfh_pair_features(ni, nj, d, r2, &c, &s, &a, &f);
    if (!frame) return false;
    ch[0] = variant == STRICT_EDGE ? theta_strict(c, s) : fpfh_bin_theta(c, s);
    ch[1] = FPFH_BINS + fpfh_bin_unit(a);
    ch[2] = 2 * FPFH_BINS + fpfh_bin_unit(f);
    return true;
}

template <typename T>
void load3(const T* p, double* v) { v[0] = (double)p[0]; v[1] = (double)p[1]; v[2] = (double)p[2]; }

template <typename I>
int neighbour(I j, int i, int rows, int variant) { return variant == KEEP_SELF ? group_row(j, rows) : fpfh_neighbour(j, i, rows); }

bool near(bool ok_i, bool ok_j, double r2, double radius2, int variant) {
    if (variant == KEEP_SELF) return ok_i && ok_j && (radius2 < 0.0 || r2 <= radius2);
    return fpfh_near(ok_i, ok_j, r2, radius2);
}

// the two passes of csrc/fpfh.hip, one row and one slot after the other
template <typename T, typename I>
void cloud(const T* pts, int c, const T* nrm, const I* idx, const T* sd2, int m, int rows, int k, double radius, int variant, uint8_t* cnt, T* out) {
    const double radius2 = radius == 0.0 ? -1.0 : radius * radius;
    std::vector<uint8_t> ok((size_t)m, 0);
    std::vector<int> np((size_t)m, 0);
    for (int i = 0; i < m; ++i) {
        for (int ch = 0; ch < FPFH_CH; ++ch) cnt[(size_t)i * FPFH_CH + ch] = 0;
        if (i >= rows) continue;
        double pi[3], ni[3];
        load3(pts + (size_t)i * c, pi);
        load3(nrm + (size_t)i * 3, ni);
        ok[(size_t)i] = fpfh_row_ok(pi, ni);
    }
    for (int i = 0; i < rows; ++i) {
        if (!ok[(size_t)i]) continue;
        double pi[3], ni[3];
        load3(pts + (size_t)i * c, pi);
        load3(nrm + (size_t)i * 3, ni);
        for (int s = 0; s < k; ++s) {
            const int j = neighbour(idx[(size_t)i * k + s], i, rows, variant);
            if (j < 0) continue;
            double pj[3], nj[3], d[3];
            load3(pts + (size_t)j * c, pj);
            load3(nrm + (size_t)j * 3, nj);
            const double r2 = fpfh_d2(pi, pj, d);
            int ch[3];
            if (near(true, ok[(size_t)j] != 0, r2, radius2, variant) && pair_bins(ni, nj, d, r2, variant, ch)) {
                for (int a = 0; a < 3; ++a) ++cnt[(size_t)i * FPFH_CH + ch[a]];
                ++np[(size_t)i];
            }
        }
    }
    for (int i = 0; i < m; ++i) {
        double acc[FPFH_CH];
        for (int ch = 0; ch < FPFH_CH; ++ch) acc[ch] = 0.0;
        if (i < rows && ok[(size_t)i]) {
            double pi[3];
            load3(pts + (size_t)i * c, pi);
            for (int s = 0; s < k; ++s) {
                const int j = neighbour(idx[(size_t)i * k + s], i, rows, variant);
                if (j < 0) continue;
                double pj[3], d[3];
                load3(pts + (size_t)j * c, pj);
                const double r2 = fpfh_d2(pi, pj, d);
                if (!near(true, ok[(size_t)j] != 0, r2, radius2, variant)) continue;
                const double wt = fpfh_weight(variant == SEARCH_D2 ? (double)sd2[(size_t)i * k + s] : r2);
                const int cj = variant == NORM_K ? (np[(size_t)j] > 0 ? k : 0) : np[(size_t)j];
                for (int ch = 0; ch < FPFH_CH; ++ch) acc[ch] = fpfh_weight_add(acc[ch], wt, fpfh_spfh(cnt[(size_t)j * FPFH_CH + ch], cj));
            }
        }
        const int ci = variant == NORM_K ? (np[(size_t)i] > 0 ? k : 0) : np[(size_t)i];
        for (int g = 0; g < 3; ++g) {
            double S = 0.0;
            for (int a = 0; a < FPFH_BINS; ++a) S = S + acc[g * FPFH_BINS + a];
            for (int a = 0; a < FPFH_BINS; ++a) {
                const int ch = g * FPFH_BINS + a;
                out[(size_t)i * FPFH_CH + ch] = (T)fpfh_out(acc[ch], S, fpfh_spfh(cnt[(size_t)i * FPFH_CH + ch], ci));
            }
        }
    }
}

template <typename T>
void cloud_i(int idx64, const void* pts, int c, const void* nrm, const void* idx, const void* sd2, int m, int rows, int k, double radius, int variant,
             uint8_t* cnt, void* out) {
    if (idx64) cloud<T, int64_t>((const T*)pts, c, (const T*)nrm, (const int64_t*)idx, (const T*)sd2, m, rows, k, radius, variant, cnt, (T*)out);
    else cloud<T, int32_t>((const T*)pts, c, (const T*)nrm, (const int32_t*)idx, (const T*)sd2, m, rows, k, radius, variant, cnt, (T*)out);
}

}  // namespace

extern "C" {

// FPFH_BINS, FPFH_CH, FPFH_K_MIN, FPFH_K_MAX, FPFH_ROW_BYTES
void fpc_constants(int32_t* out) {
    out[0] = FPFH_BINS; out[1] = FPFH_CH; out[2] = FPFH_K_MIN; out[3] = FPFH_K_MAX; out[4] = FPFH_ROW_BYTES;
}

// the bins of n values: theta from (c, s), and fpfh_bin_unit of a
void fpc_bins(const double* c, const double* s, const double* a, int n, int32_t* theta, int32_t* unit) {
    for (int i = 0; i < n; ++i) { theta[i] = fpfh_bin_theta(c[i], s[i]); unit[i] = fpfh_bin_unit(a[i]); }
}

// one cloud.  sd2: the search's d2 (m, k) in the points' type, read by variant 4 only.  radius 0: none.
void fpc_cloud(int f64, int idx64, const void* pts, int c, const void* nrm, const void* idx, const void* sd2, int m, int rows, int k, double radius,
               int variant, uint8_t* cnt, void* out) {
    if (f64) cloud_i<double>(idx64, pts, c, nrm, idx, sd2, m, rows, k, radius, variant, cnt, out);
    else cloud_i<float>(idx64, pts, c, nrm, idx, sd2, m, rows, k, radius, variant, cnt, out);
}

}
