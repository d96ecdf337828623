// TEST-ONLY host build of dicp_amd/csrc/dicp_compat.h (g++, no GPU): the two fma chains, the square roots, the relation, the degree, the
// power iteration with its sequential sums and the ranks -- the lines the HIP kernels execute -- run in a serial loop over one cloud's
// packed pairs, for tests/test_compat_host.py.  Never loaded by dicp_amd.
#include <stdint.h>

#include <vector>

#include "../../dicp_amd/csrc/dicp_compat.h"

using namespace dicp;

namespace {

template <typename T>
bool pair_of(const T* pairs, int p, int q, T thr, T L) {
    const T* a = pairs + (size_t)p * COMPAT_ROW;
    const T* b = pairs + (size_t)q * COMPAT_ROW;
    return compat_pair<T>(a[0], a[1], a[2], a[3], a[4], a[5], b[0], b[1], b[2], b[3], b[4], b[5], thr, L);
}

// A, B, e (P, P) and the relation (P, P) bytes, the diagonal included
template <typename T>
void relation(const T* pairs, int P, double threshold, double min_length, T* A, T* B, T* e, uint8_t* rel) {
    const T thr = compat_thr<T>(threshold), L = compat_thr<T>(min_length);
    for (int p = 0; p < P; ++p)
        for (int q = 0; q < P; ++q) {
            const T* a = pairs + (size_t)p * COMPAT_ROW;
            const T* b = pairs + (size_t)q * COMPAT_ROW;
            const size_t o = (size_t)p * P + q;
            A[o] = compat_len2<T>(a[0], a[1], a[2], b[0], b[1], b[2]);
            B[o] = compat_len2<T>(a[3], a[4], a[5], b[3], b[4], b[5]);
            T la, lb;
            e[o] = compat_error<T>(A[o], B[o], la, lb);
            rel[o] = pair_of<T>(pairs, p, q, thr, L) ? 1 : 0;
        }
}

// degree (P), w and v of every iteration (iterations, P)
template <typename T>
void scores(const T* pairs, int P, int iterations, double threshold, double min_length, int32_t* degree, T* w, T* v) {
    const T thr = compat_thr<T>(threshold), L = compat_thr<T>(min_length);
    std::vector<T> cur((size_t)P, T(1));
    for (int p = 0; p < P; ++p) {
        int32_t d = 0;
        for (int q = 0; q < P; ++q) d += (q != p && pair_of<T>(pairs, p, q, thr, L)) ? 1 : 0;
        degree[p] = d;
    }
    for (int it = 0; it < iterations; ++it) {
        T* wi = w + (size_t)it * P;
        T* vi = v + (size_t)it * P;
        T wmax = T(0);
        for (int p = 0; p < P; ++p) {
            T s = T(0);
            for (int q = 0; q < P; ++q) s = s + compat_term<T>(q == p, pair_of<T>(pairs, p, q, thr, L), cur[q]);
            wi[p] = s;
            wmax = s > wmax ? s : wmax;
        }
        for (int p = 0; p < P; ++p) vi[p] = compat_div<T>(wi[p], wmax);
        for (int p = 0; p < P; ++p) cur[p] = vi[p];
    }
}

template <typename T>
void rank_of(const T* score, int P, int32_t* rank) {
    for (int p = 0; p < P; ++p) {
        int32_t r = 0;
        for (int q = 0; q < P; ++q) r += compat_before<T>(score[q], q, score[p], p) ? 1 : 0;
        rank[p] = r;
    }
}

}  // namespace

extern "C" {

int cc_iter_max() { return COMPAT_ITER_MAX; }
void cc_relation_f32(const float* pairs, int P, double thr, double L, float* A, float* B, float* e, uint8_t* rel) { relation<float>(pairs, P, thr, L, A, B, e, rel); }
void cc_relation_f64(const double* pairs, int P, double thr, double L, double* A, double* B, double* e, uint8_t* rel) { relation<double>(pairs, P, thr, L, A, B, e, rel); }
void cc_scores_f32(const float* pairs, int P, int it, double thr, double L, int32_t* degree, float* w, float* v) { scores<float>(pairs, P, it, thr, L, degree, w, v); }
void cc_scores_f64(const double* pairs, int P, int it, double thr, double L, int32_t* degree, double* w, double* v) { scores<double>(pairs, P, it, thr, L, degree, w, v); }
void cc_rank_f32(const float* score, int P, int32_t* rank) { rank_of<float>(score, P, rank); }
void cc_rank_f64(const double* score, int P, int32_t* rank) { rank_of<double>(score, P, rank); }

}
