// TEST-ONLY host build of dicp_amd/csrc/dicp_match.h (g++, no GPU): the score chain, h, the candidate rule, the (score, index) list, the
// refined d2 and the two gradients -- the lines the HIP kernels execute (match_fma is __builtin_fmaf / __builtin_fma) -- run in a serial
// loop over one cloud, for tests/test_match_host.py.  Never loaded by dicp_amd.
#include <stdint.h>

#include <vector>

#include "../../dicp_amd/csrc/dicp_match.h"

using namespace dicp;

namespace {

template <typename T>
void knn(const T* x, int n, int x_rows, const T* y, int m, int y_rows, int D, int k, T* h, T* score_all, T* d2, int64_t* idx, T* sc_out) {
    for (int j = 0; j < m; ++j) h[j] = match_half_norm<T>(y + (size_t)j * D, D);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j) score_all[(size_t)i * m + j] = match_score<T>(x + (size_t)i * D, y + (size_t)j * D, D, h[j]);
    topk_with_kcap(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        for (int i = 0; i < n; ++i) {
            T sc[K];
            int id[K], sl[K];
            topk_init<T, K>(sc, id, sl, k);
            if (i < x_rows) match_query<T, K>(x + (size_t)i * D, y, h, y_rows, D, k, sc, id);
            for (int e = K - k; e < K; ++e) {
                const size_t o = (size_t)i * k + (e - (K - k));
                match_output<T>(x + (size_t)i * D, y, D, id[e], d2[o], idx[o]);
                sc_out[o] = sc[e];
            }
        }
    });
}

template <typename T>
void grads(const T* g, const int64_t* idx, const T* x, int n, const T* y, int m, int rows, int D, int k, const int32_t* offsets, const int32_t* slots,
           T* gx, T* gy) {
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < D; ++c) gx[(size_t)i * D + c] = match_grad_x<T>(g + (size_t)i * k, idx + (size_t)i * k, k, x[(size_t)i * D + c], y, D, m, c);
    for (int j = 0; j < m; ++j) {
        int lo = 0, hi = 0;
        if (j < rows) det_list(offsets, j, n * k, lo, hi);
        for (int c = 0; c < D; ++c) gy[(size_t)j * D + c] = match_det_sum<T>(g, idx, x, n, k, D, rows, slots, j, y[(size_t)j * D + c], c, lo, hi);
    }
}

}  // namespace

extern "C" {

int mc_chunk() { return GROUP_DET_CHUNK; }
int mc_d_max() { return MATCH_D_MAX; }

void mc_knn_f32(const float* x, int n, int x_rows, const float* y, int m, int y_rows, int D, int k, float* h, float* score_all, float* d2, int64_t* idx,
                float* sc) { knn<float>(x, n, x_rows, y, m, y_rows, D, k, h, score_all, d2, idx, sc); }
void mc_knn_f64(const double* x, int n, int x_rows, const double* y, int m, int y_rows, int D, int k, double* h, double* score_all, double* d2,
                int64_t* idx, double* sc) { knn<double>(x, n, x_rows, y, m, y_rows, D, k, h, score_all, d2, idx, sc); }
void mc_grads_f32(const float* g, const int64_t* idx, const float* x, int n, const float* y, int m, int rows, int D, int k, const int32_t* offsets,
                  const int32_t* slots, float* gx, float* gy) { grads<float>(g, idx, x, n, y, m, rows, D, k, offsets, slots, gx, gy); }
void mc_grads_f64(const double* g, const int64_t* idx, const double* x, int n, const double* y, int m, int rows, int D, int k, const int32_t* offsets,
                  const int32_t* slots, double* gx, double* gy) { grads<double>(g, idx, x, n, y, m, rows, D, k, offsets, slots, gx, gy); }
float mc_fmaf(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
double mc_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

}
