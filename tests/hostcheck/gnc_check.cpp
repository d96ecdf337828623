// TEST-ONLY host build of dicp_amd/csrc/dicp_gnc.h (g++, no GPU): the residual, the weights, the sums in the header's tree, the fit and
// the stopping rules -- the lines the HIP kernel executes -- run in a serial loop over one cloud's packed pairs, for
// tests/test_gnc_host.py and tests/test_gpu_gnc.py.  Never loaded by dicp_amd.
#include <stdint.h>

#include <vector>

#include "../../dicp_amd/csrc/dicp_gnc.h"

using namespace dicp;

namespace {

// F(w): the slots' sequential partials, the tree, kabsch_forward -> sums (18), pose (12)
template <typename T>
void fit(const T* pairs, int P, const T* u, const double* w, std::vector<double>& slots, double* sums, double* pose) {
    slots.assign((size_t)GNC_SLOTS * NKAB, 0.0);
    for (int p = 0; p < P; ++p) {
        const double wp = w ? w[p] : 1.0;
        const double omega = u ? (double)u[p] * wp : wp;
        if (omega > 0.0) gnc_add<T>(&slots[(size_t)(p % GNC_SLOTS) * NKAB], omega, pairs + (size_t)p * GNC_ROW);
    }
    gnc_tree(slots.data(), GNC_SLOTS, NKAB);
    for (int k = 0; k < NKAB; ++k) sums[k] = slots[k];
    double C[9], r[3], save[KAB_SAVE];
    kabsch_forward(sums, C, r, save);
    for (int k = 0; k < 9; ++k) pose[k] = C[k];
    for (int k = 0; k < 3; ++k) pose[9 + k] = r[k];
}

void record(double* trace, int k, double mu, double band, const double* sums, const double* pose) {
    if (!trace) return;
    double* t = trace + (size_t)k * GNC_TRACE;
    t[0] = mu; t[1] = band;
    for (int i = 0; i < NKAB; ++i) t[2 + i] = sums[i];
    for (int i = 0; i < 12; ++i) t[2 + NKAB + i] = pose[i];
}

// dicp_gnc_fit for one cloud.  detail: optional (iterations + 1, 2, P) doubles: for applied round k the residuals its weights were formed
// from, then the weights (record 0: zeros, ones).
template <typename T>
int run(const T* pairs, int P, const T* u, int loss, double threshold, double growth, int iterations, T* weights, int32_t* rounds, int32_t* status, double* mu,
        T* pose_last, double* trace, double* detail) {
    if (gnc_bad_arguments(loss, threshold, growth, iterations)) return 2;
    const double c2 = threshold * threshold;
    double pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, sums[NKAB];
    if (P < 3) {
        for (int p = 0; p < P; ++p) weights[p] = T(0);
        *rounds = 0; *status = GNC_TOO_FEW; *mu = 0.0;
        for (int k = 0; k < 12; ++k) pose_last[k] = (T)pose[k];
        return 0;
    }
    std::vector<double> slots, w((size_t)P, 1.0), wn((size_t)P), d((size_t)P);
    fit<T>(pairs, P, u, nullptr, slots, sums, pose);
    record(trace, 0, 0.0, 0.0, sums, pose);
    if (detail)
        for (int p = 0; p < P; ++p) { detail[p] = 0.0; detail[(size_t)P + p] = 1.0; }
    double dmax = 0.0;
    for (int p = 0; p < P; ++p) {
        const double v = gnc_residual<T>(pose, pairs + (size_t)p * GNC_ROW);
        if (v < gnc_inf() && v > dmax) dmax = v;
    }
    GncState st;
    gnc_begin(loss, dmax, c2, st);
    for (int it = 0; it < iterations && st.go; ++it) {
        const GncRound rd = gnc_round(loss, st.mu, c2);
        int64_t npos = 0, band = 0;
        for (int p = 0; p < P; ++p) {
            int b;
            d[p] = gnc_residual<T>(pose, pairs + (size_t)p * GNC_ROW);
            wn[p] = gnc_weight(rd, d[p], b);
            const double omega = u ? (double)u[p] * wn[p] : wn[p];
            npos += omega > 0.0 ? 1 : 0;
            band += b;
        }
        if (!gnc_apply(loss, npos, band, growth, iterations, st)) break;
        w = wn;
        fit<T>(pairs, P, u, w.data(), slots, sums, pose);
        record(trace, st.rounds, st.mu_used, (double)band, sums, pose);
        if (detail)
            for (int p = 0; p < P; ++p) { detail[((size_t)st.rounds * 2) * P + p] = d[p]; detail[((size_t)st.rounds * 2 + 1) * P + p] = w[p]; }
    }
    for (int p = 0; p < P; ++p) weights[p] = (T)w[p];
    *rounds = st.rounds; *status = st.status; *mu = st.mu_used;
    for (int k = 0; k < 12; ++k) pose_last[k] = (T)pose[k];
    return 0;
}

}  // namespace

extern "C" {

int gc_slots() { return GNC_SLOTS; }
int gc_iter_max() { return GNC_ITER_MAX; }
int gc_trace() { return GNC_TRACE; }
int gc_bad_arguments(int loss, double threshold, double growth, int iterations) { return gnc_bad_arguments(loss, threshold, growth, iterations) ? 1 : 0; }
double gc_residual_f32(const double* pose, const float* row) { return gnc_residual<float>(pose, row); }
double gc_residual_f64(const double* pose, const double* row) { return gnc_residual<double>(pose, row); }
// out: lo, hi, w, band of one pair at (loss, mu, c2)
void gc_weight(int loss, double mu, double c2, double d, double* out) {
    const GncRound rd = gnc_round(loss, mu, c2);
    int b;
    out[2] = gnc_weight(rd, d, b);
    out[0] = rd.lo; out[1] = rd.hi; out[3] = (double)b;
}
int gc_fit_f32(const float* pairs, int P, const float* u, int loss, double threshold, double growth, int iterations, float* weights, int32_t* rounds,
               int32_t* status, double* mu, float* pose_last, double* trace, double* detail) {
    return run<float>(pairs, P, u, loss, threshold, growth, iterations, weights, rounds, status, mu, pose_last, trace, detail);
}
int gc_fit_f64(const double* pairs, int P, const double* u, int loss, double threshold, double growth, int iterations, double* weights, int32_t* rounds,
               int32_t* status, double* mu, double* pose_last, double* trace, double* detail) {
    return run<double>(pairs, P, u, loss, threshold, growth, iterations, weights, rounds, status, mu, pose_last, trace, detail);
}

}
