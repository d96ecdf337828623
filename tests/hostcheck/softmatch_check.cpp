// TEST-ONLY host build of dicp_amd/csrc/dicp_softmatch.h (g++, no GPU): the online softmax over the exact scores, the hard winner and the
// three gradients -- the lines the HIP kernels execute, in the vector kernels' order -- run in a serial loop over one cloud, for
// tests/test_softmatch_host.py.  Never loaded by dicp_amd.
#include <stdint.h>

#include <vector>

#include "../../dicp_amd/csrc/dicp_softmatch.h"

using namespace dicp;

namespace {

constexpr int CC = SOFT_C_MAX;

template <typename T>
void forward(const T* x, int n, int x_rows, const T* y, int m, int y_rows, int D, const T* values, int C, double tau, T* out, T* lse, int64_t* idx,
             T* prob) {
    std::vector<T> h(m);
    for (int j = 0; j < m; ++j) h[j] = match_half_norm<T>(y + (size_t)j * D, D);
    const T c = soft_scale<T>(tau);
    for (int i = 0; i < n; ++i)
        soft_query<T, CC>(x + (size_t)i * D, y, h.data(), values, i < x_rows ? y_rows : 0, D, C, c, out + (size_t)i * C, lse[i], idx[i], prob[i]);
}

template <typename T>
void backward(const T* x, int n, int x_rows, const T* y, int m, int y_rows, int D, const T* values, int C, double tau, const T* out, const T* lse,
              const T* g, T* gx, T* gy, T* gv) {
    std::vector<T> h(m), delta(n), go((size_t)n * CC, T(0)), vv((size_t)m * CC, T(0));
    for (int j = 0; j < m; ++j) h[j] = match_half_norm<T>(y + (size_t)j * D, D);
    const T c = soft_scale<T>(tau);
    for (int j = 0; j < y_rows; ++j)
        for (int k = 0; k < C; ++k) vv[(size_t)j * CC + k] = values[(size_t)j * C + k];
    for (int i = 0; i < n; ++i) {
        T o[CC] = {};
        for (int k = 0; k < C; ++k) { go[(size_t)i * CC + k] = g[(size_t)i * C + k]; o[k] = out[(size_t)i * C + k]; }
        delta[i] = soft_dot<T, CC>(go.data() + (size_t)i * CC, o);
    }
    const auto term = [&](int i, int j, T& p, T& a) {
        if (i >= x_rows || j >= y_rows || !soft_live<T>(lse[i])) return false;
        const T s = match_score<T>(x + (size_t)i * D, y + (size_t)j * D, D, h[j]);
        if (!match_finite<T>(s)) return false;
        p = soft_prob<T>(c, s, lse[i]);
        a = soft_a<T>(p, soft_dot<T, CC>(go.data() + (size_t)i * CC, vv.data() + (size_t)j * CC), delta[i]);
        return true;
    };
    for (int i = 0; i < n; ++i) {
        std::vector<T> G(D, T(0));
        for (int j = 0; j < m; ++j) {
            T p, a;
            if (!term(i, j, p, a)) continue;
            for (int ch = 0; ch < D; ++ch) G[ch] = match_fma(a, y[(size_t)j * D + ch], G[ch]);
        }
        const bool on = i < x_rows && soft_live<T>(lse[i]);
        for (int ch = 0; ch < D; ++ch) gx[(size_t)i * D + ch] = on ? soft_grad_x<T>(c, G[ch]) : T(0);
    }
    for (int j = 0; j < m; ++j) {
        std::vector<T> A(D, T(0));
        T sa = T(0), GV[CC] = {};
        bool any = false;
        for (int i = 0; i < n; ++i) {
            T p, a;
            if (!term(i, j, p, a)) continue;
            any = true;
            sa = sa + a;
            for (int k = 0; k < CC; ++k) GV[k] = match_fma(p, go[(size_t)i * CC + k], GV[k]);
            for (int ch = 0; ch < D; ++ch) A[ch] = match_fma(a, x[(size_t)i * D + ch], A[ch]);
        }
        for (int ch = 0; ch < D; ++ch) gy[(size_t)j * D + ch] = any ? soft_grad_y<T>(c, y[(size_t)j * D + ch], sa, A[ch]) : T(0);
        for (int k = 0; k < C; ++k) gv[(size_t)j * C + k] = any ? GV[k] : T(0);
    }
}

}  // namespace

extern "C" {

int sc_rows() { return SOFT_ROWS; }
int sc_c_max() { return SOFT_C_MAX; }

void sc_forward_f32(const float* x, int n, int x_rows, const float* y, int m, int y_rows, int D, const float* values, int C, double tau, float* out,
                    float* lse, int64_t* idx, float* prob) { forward<float>(x, n, x_rows, y, m, y_rows, D, values, C, tau, out, lse, idx, prob); }
void sc_forward_f64(const double* x, int n, int x_rows, const double* y, int m, int y_rows, int D, const double* values, int C, double tau, double* out,
                    double* lse, int64_t* idx, double* prob) { forward<double>(x, n, x_rows, y, m, y_rows, D, values, C, tau, out, lse, idx, prob); }
void sc_backward_f32(const float* x, int n, int x_rows, const float* y, int m, int y_rows, int D, const float* values, int C, double tau, const float* out,
                     const float* lse, const float* g, float* gx, float* gy, float* gv) {
    backward<float>(x, n, x_rows, y, m, y_rows, D, values, C, tau, out, lse, g, gx, gy, gv);
}
void sc_backward_f64(const double* x, int n, int x_rows, const double* y, int m, int y_rows, int D, const double* values, int C, double tau, const double* out,
                     const double* lse, const double* g, double* gx, double* gy, double* gv) {
    backward<double>(x, n, x_rows, y, m, y_rows, D, values, C, tau, out, lse, g, gx, gy, gv);
}

}  // extern "C"
