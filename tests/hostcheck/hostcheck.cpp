// TEST-ONLY host build of dicp_amd/csrc/dicp_math.h (g++, no GPU).
// Lets the CPU test-suite check the closed-form forward/backward formulas that the
// HIP kernels execute against the oracle's autograd.  Never loaded by dicp_amd.
#include "../../dicp_amd/csrc/dicp_math.h"

using namespace dicp;

template <typename T>
static void forward_t(const WeightParams& P, int n, int c, const T* src, const T* tgt, const int* idx,
                      const T* C, const T* r, const T* w0, T* acc, T* w_out) {
    for (int k = 0; k < NACC; ++k) acc[k] = T(0);
    const T zero3[3] = {T(0), T(0), T(0)};
    for (int i = 0; i < n; ++i) {
        const T* y = tgt + (long)idx[i] * c;
        PointState<T> s;
        if (P.mode == MODE_PT2PL) point_forward<T, MODE_PT2PL>(P, C, r, src + 3 * i, y, y + 3, w0[i], acc, s);
        else                      point_forward<T, MODE_PT2PT>(P, C, r, src + 3 * i, y, zero3, w0[i], acc, s);
        w_out[i] = s.w;
    }
}

template <typename T>
static void backward_t(const WeightParams& P, int n, int c, const T* src, const T* tgt, const int* idx,
                       const T* C, const T* r, const T* w0, const T* Gs, const T* gb,
                       T* gsrc, T* gtgt, T* gw0, T* gC, T* gr) {
    const T zero3[3] = {T(0), T(0), T(0)};
    for (int i = 0; i < n; ++i) {
        const T* y = tgt + (long)idx[i] * c;
        T gp[3], gy[3], gn[3], gw;
        if (P.mode == MODE_PT2PL) point_backward<T, MODE_PT2PL>(P, C, r, src + 3 * i, y, y + 3, w0[i], Gs, gb, gp, gy, gn, gw, gC, gr);
        else                      point_backward<T, MODE_PT2PT>(P, C, r, src + 3 * i, y, zero3, w0[i], Gs, gb, gp, gy, gn, gw, gC, gr);
        for (int k = 0; k < 3; ++k) { gsrc[3 * i + k] += gp[k]; gtgt[(long)idx[i] * c + k] += gy[k]; }
        if (c == 6) for (int k = 0; k < 3; ++k) gtgt[(long)idx[i] * c + 3 + k] += gn[k];
        gw0[i] += gw;
    }
}

// One point per cloud, each with its own pose (N,12) = [C row-major | r]: the per-point values the operator-level tests hold to
// tests/point_math_ref.py.  acc (N,30), gpose (N,12) = [C-bar | r-bar]; every output is overwritten.
template <typename T>
static void points_forward_t(const WeightParams& P, int N, int c, const T* src, const T* tgt, const T* pose, const T* w0, T* acc, T* w_out) {
    const int zero = 0;
    for (int i = 0; i < N; ++i) forward_t<T>(P, 1, c, src + 3 * i, tgt + (long)c * i, &zero, pose + 12 * i, pose + 12 * i + 9, w0 + i, acc + (long)NACC * i, w_out + i);
}
template <typename T>
static void points_backward_t(const WeightParams& P, int N, int c, const T* src, const T* tgt, const T* pose, const T* w0, const T* Gs, const T* gb,
                              T* gsrc, T* gtgt, T* gw0, T* gpose) {
    const int zero = 0;
    for (int i = 0; i < N; ++i) {
        for (int k = 0; k < 3; ++k) gsrc[3 * i + k] = T(0);
        for (int k = 0; k < c; ++k) gtgt[(long)c * i + k] = T(0);
        for (int k = 0; k < 12; ++k) gpose[12 * i + k] = T(0);
        gw0[i] = T(0);
        backward_t<T>(P, 1, c, src + 3 * i, tgt + (long)c * i, &zero, pose + 12 * i, pose + 12 * i + 9, w0 + i, Gs + 36 * i, gb + 6 * i,
                      gsrc + 3 * i, gtgt + (long)c * i, gw0 + i, gpose + 12 * i, gpose + 12 * i + 9);
    }
}

// The stand-alone loss weight and its backward (loss_eval / loss_weight{,_bwd}_kernel of csrc/kernels_soft_svd.h, which only a HIP compiler can
// include), restated call for call on the m_* functions of dicp_math.h: m_sqrt, m_tanh and plain '/'.  tests/test_point_math_ref.py holds the
// kernels' text to this restatement's operations.  loss: 1 huber, 2 cauchy, 3 trim.
template <typename T>
static void loss_eval_t(int loss, int diff, T metric, T kk, const T* e, int r, T& w, T& en, T& th) {
    T s = T(0);
    for (int k = 0; k < r; ++k) s += e[k] * e[k];
    en = m_sqrt(s);
    th = T(0);
    if (loss == LOSS_HUBER) {
        if (diff) w = (metric * metric) / (metric * metric + en * en);
        else      w = (en > metric) ? metric / en : T(1);
    } else if (loss == LOSS_CAUCHY) {
        const T t = en / metric;
        w = T(1) / (T(1) + t * t);
    } else {
        if (diff) { th = m_tanh(kk * (metric - en) - T(3)); w = T(0.5) * th + T(0.5); }
        else      w = (en < metric) ? T(1) : T(0);
    }
}
template <typename T>
static void loss_weight_t(int loss, int diff, double metric, double kk, const T* err, long rows, int r, T* w) {
    for (long i = 0; i < rows; ++i) {
        T en, th;
        loss_eval_t<T>(loss, diff, (T)metric, (T)kk, err + i * r, r, w[i], en, th);
    }
}
template <typename T>
static void loss_weight_bwd_t(int loss, int diff, double metric_d, double kk_d, const T* err, const T* gw, long rows, int r, T* gerr) {
    const T metric = (T)metric_d, kk = (T)kk_d;
    for (long i = 0; i < rows; ++i) {
        const T* e = err + i * r;
        T wv, en, th;
        loss_eval_t<T>(loss, diff, metric, kk, e, r, wv, en, th);
        T dw = T(0);
        if (loss == LOSS_HUBER) {
            if (diff) dw = -T(2) * en * wv * wv / (metric * metric);
            else      dw = hard_huber_slope(en, metric);
        } else if (loss == LOSS_CAUCHY) {
            dw = -T(2) * en * wv * wv / (metric * metric);
        } else if (diff) {
            dw = -T(0.5) * kk * (T(1) - th * th);
        }
        for (int k = 0; k < r; ++k) gerr[i * r + k] = (en > T(0)) ? gw[i] * dw * e[k] / en : gw[i] * dw * T(0);
    }
}

extern "C" {

void hc_backward_f32(const WeightParams* P, int n, int c, const float* src, const float* tgt, const int* idx,
                     const float* C, const float* r, const float* w0, const float* Gs, const float* gb,
                     float* gsrc, float* gtgt, float* gw0, float* gC, float* gr) {
    backward_t<float>(*P, n, c, src, tgt, idx, C, r, w0, Gs, gb, gsrc, gtgt, gw0, gC, gr);
}
void hc_points_forward_f32(const WeightParams* P, int N, int c, const float* src, const float* tgt, const float* pose, const float* w0, float* acc, float* w_out) {
    points_forward_t<float>(*P, N, c, src, tgt, pose, w0, acc, w_out);
}
void hc_points_forward_f64(const WeightParams* P, int N, int c, const double* src, const double* tgt, const double* pose, const double* w0, double* acc, double* w_out) {
    points_forward_t<double>(*P, N, c, src, tgt, pose, w0, acc, w_out);
}
void hc_points_backward_f32(const WeightParams* P, int N, int c, const float* src, const float* tgt, const float* pose, const float* w0, const float* Gs, const float* gb,
                            float* gsrc, float* gtgt, float* gw0, float* gpose) {
    points_backward_t<float>(*P, N, c, src, tgt, pose, w0, Gs, gb, gsrc, gtgt, gw0, gpose);
}
void hc_points_backward_f64(const WeightParams* P, int N, int c, const double* src, const double* tgt, const double* pose, const double* w0, const double* Gs, const double* gb,
                            double* gsrc, double* gtgt, double* gw0, double* gpose) {
    points_backward_t<double>(*P, N, c, src, tgt, pose, w0, Gs, gb, gsrc, gtgt, gw0, gpose);
}
void hc_loss_weight_f32(int loss, int diff, double metric, double kk, const float* err, long rows, int r, float* w) { loss_weight_t<float>(loss, diff, metric, kk, err, rows, r, w); }
void hc_loss_weight_f64(int loss, int diff, double metric, double kk, const double* err, long rows, int r, double* w) { loss_weight_t<double>(loss, diff, metric, kk, err, rows, r, w); }
void hc_loss_weight_bwd_f32(int loss, int diff, double metric, double kk, const float* err, const float* gw, long rows, int r, float* gerr) {
    loss_weight_bwd_t<float>(loss, diff, metric, kk, err, gw, rows, r, gerr);
}
void hc_loss_weight_bwd_f64(int loss, int diff, double metric, double kk, const double* err, const double* gw, long rows, int r, double* gerr) {
    loss_weight_bwd_t<double>(loss, diff, metric, kk, err, gw, rows, r, gerr);
}
void hc_forward_f64(const WeightParams* P, int n, int c, const double* src, const double* tgt, const int* idx,
                    const double* C, const double* r, const double* w0, double* acc, double* w_out) {
    forward_t<double>(*P, n, c, src, tgt, idx, C, r, w0, acc, w_out);
}
void hc_forward_f32(const WeightParams* P, int n, int c, const float* src, const float* tgt, const int* idx,
                    const float* C, const float* r, const float* w0, float* acc, float* w_out) {
    forward_t<float>(*P, n, c, src, tgt, idx, C, r, w0, acc, w_out);
}
void hc_backward_f64(const WeightParams* P, int n, int c, const double* src, const double* tgt, const int* idx,
                     const double* C, const double* r, const double* w0, const double* Gs, const double* gb,
                     double* gsrc, double* gtgt, double* gw0, double* gC, double* gr) {
    backward_t<double>(*P, n, c, src, tgt, idx, C, r, w0, Gs, gb, gsrc, gtgt, gw0, gC, gr);
}
void hc_step_forward(const double* acc, int dim, const double* C, const double* r,
                     double* delta6, double* Cn, double* rn, double* Areg) {
    double A6[36];
    unpack_sym6(acc + ACC_A, A6);
    step_forward(A6, acc + ACC_B, dim, C, r, delta6, Cn, rn, Areg);
}
void hc_step_backward(const double* gCn, const double* grn, int dim, const double* C, const double* delta6,
                      const double* Areg, double* Gs, double* gb, double* gC, double* gr) {
    step_backward(gCn, grn, dim, C, delta6, Areg, Gs, gb, gC, gr);
}
double hc_kabsch_forward(const double* acc, double* C, double* r, double* save) { return kabsch_forward(acc, C, r, save); }
void hc_kabsch_backward(const double* gC, const double* gr, const double* save, double* gacc) { kabsch_backward(gC, gr, save, gacc); }
void hc_svd3(const double* A, double* U, double* S, double* V) { svd3(A, U, S, V); }
int hc_sizeof_params() { return (int)sizeof(WeightParams); }

}  // extern "C"
