// TEST-ONLY host build of dicp_amd/csrc/dicp_ransac.h (g++, no GPU): the hash and the sampler, the sums in front of kabsch_forward and
// the fit, the residual chain, the counts and the (count, h) choice -- the lines the HIP kernels execute -- run in a serial loop over one
// cloud's packed pairs, for tests/test_ransac_host.py.  Never loaded by dicp_amd.
#include <stdint.h>

#include "../../dicp_amd/csrc/dicp_ransac.h"

using namespace dicp;

namespace {

template <typename T>
void hypotheses(const T* pairs, int P, int H, uint32_t seed, uint32_t cloud, int32_t* samples, double* sums, T* poses) {
    for (int h = 0; h < H; ++h) {
        int32_t a, b, c;
        ransac_sample(seed, cloud, (uint32_t)h, (uint32_t)P, a, b, c);
        samples[3 * h] = a; samples[3 * h + 1] = b; samples[3 * h + 2] = c;
        double acc[NKAB];
        ransac_sums<T>(pairs + (size_t)a * RANSAC_ROW, pairs + (size_t)b * RANSAC_ROW, pairs + (size_t)c * RANSAC_ROW, acc);
        for (int i = 0; i < NKAB; ++i) sums[(size_t)h * NKAB + i] = acc[i];
        T pose[12];
        ransac_fit<T>(pairs + (size_t)a * RANSAC_ROW, pairs + (size_t)b * RANSAC_ROW, pairs + (size_t)c * RANSAC_ROW, pose);
        for (int i = 0; i < 12; ++i) poses[(size_t)h * 12 + i] = pose[i];
    }
}

// d (H, P), counts (H), best / best_count of one cloud's packed pairs under H poses
template <typename T>
void score(const T* pairs, int P, const T* poses, int H, double threshold, T* d, int32_t* counts, int32_t* best, int32_t* best_count) {
    const T thr2 = ransac_thr2<T>(threshold);
    int32_t bc = -1, bh = 0x7fffffff;
    for (int h = 0; h < H; ++h) {
        T pose[12];
        for (int i = 0; i < 12; ++i) pose[i] = poses[(size_t)h * 12 + i];
        int32_t cnt = 0;
        for (int j = 0; j < P; ++j) {
            const T* r = pairs + (size_t)j * RANSAC_ROW;
            const T v = ransac_residual<T>(pose, r[0], r[1], r[2], r[3], r[4], r[5]);
            d[(size_t)h * P + j] = v;
            cnt += ransac_inlier<T>(v, thr2) ? 1 : 0;
        }
        counts[h] = cnt;
        if (ransac_better(cnt, h, bc, bh)) { bc = cnt; bh = h; }
    }
    *best = P < 3 ? -1 : bh;
    *best_count = P < 3 ? 0 : bc;
}

}  // namespace

extern "C" {

int rc_h_max() { return RANSAC_H_MAX; }
uint32_t rc_mix32(uint32_t v) { return ransac_mix32(v); }
void rc_draws(uint32_t seed, uint32_t cloud, uint32_t h, uint32_t* u) { ransac_draws(seed, cloud, h, u[0], u[1], u[2]); }
void rc_positions(uint32_t u0, uint32_t u1, uint32_t u2, uint32_t P, int32_t* abc) { ransac_positions(u0, u1, u2, P, abc[0], abc[1], abc[2]); }
void rc_hypotheses_f32(const float* pairs, int P, int H, uint32_t seed, uint32_t cloud, int32_t* samples, double* sums, float* poses) {
    hypotheses<float>(pairs, P, H, seed, cloud, samples, sums, poses);
}
void rc_hypotheses_f64(const double* pairs, int P, int H, uint32_t seed, uint32_t cloud, int32_t* samples, double* sums, double* poses) {
    hypotheses<double>(pairs, P, H, seed, cloud, samples, sums, poses);
}
void rc_score_f32(const float* pairs, int P, const float* poses, int H, double threshold, float* d, int32_t* counts, int32_t* best, int32_t* best_count) {
    score<float>(pairs, P, poses, H, threshold, d, counts, best, best_count);
}
void rc_score_f64(const double* pairs, int P, const double* poses, int H, double threshold, double* d, int32_t* counts, int32_t* best, int32_t* best_count) {
    score<double>(pairs, P, poses, H, threshold, d, counts, best, best_count);
}
int rc_live_f32(int in_rows, int64_t idx, const float* x, const float* y) { return ransac_live<float>(in_rows != 0, idx, x, y) ? 1 : 0; }
int rc_live_f64(int in_rows, int64_t idx, const double* x, const double* y) { return ransac_live<double>(in_rows != 0, idx, x, y) ? 1 : 0; }
double rc_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

}
