// TEST-ONLY host build of dicp_amd/csrc/dicp_group.h's pool rules (g++, no GPU): the maximum's update with its tie and NaN rule, the sum's
// step and the mean's division that the HIP kernels execute, run in a serial loop over one cloud, for tests/test_pool_host.py.  Never loaded by dicp_amd.
#include <stdint.h>

#include "../../dicp_amd/csrc/dicp_group.h"

using namespace dicp;

namespace {

// reduce: 0 sum, 1 mean, 2 max (include/dicp_hip.h's DICP_POOL_*)
template <typename T, typename I>
void pool(const T* f, const I* idx, int rows, int reduce, int n, int k, int C, T* out, int32_t* argmax, int32_t* counts) {
    for (int i = 0; i < n; ++i) {
        for (int c = 0; c < C; ++c) {
            T acc = T(0);
            int arg = -1, cnt = 0;
            for (int s = 0; s < k; ++s) {
                const int j = group_row(idx[(size_t)i * k + s], rows);
                if (j < 0) continue;
                ++cnt;
                const T v = f[(size_t)j * C + c];
                if (reduce == 2) pool_max_step<T>(v, j, acc, arg);
                else acc = pool_sum_step<T>(acc, v);
            }
            if (reduce == 1) acc = pool_mean<T>(acc, cnt);
            out[(size_t)i * C + c] = acc;
            argmax[(size_t)i * C + c] = arg;
            counts[i] = cnt;
        }
    }
}

}  // namespace

extern "C" {

#define PC_TYPE(T, S, I, W) \
    void pc_pool_##S##_##W(const T* f, const I* idx, int rows, int reduce, int n, int k, int C, T* out, int32_t* argmax, int32_t* counts) { \
        pool<T, I>(f, idx, rows, reduce, n, k, C, out, argmax, counts); }
PC_TYPE(float, f32, int64_t, i64)
PC_TYPE(float, f32, int32_t, i32)
PC_TYPE(double, f64, int64_t, i64)
PC_TYPE(double, f64, int32_t, i32)

// the mean's backward quotient, element by element
void pc_mean_grad_f32(const float* g, const int32_t* count, int n, float* out) { for (int i = 0; i < n; ++i) out[i] = pool_mean_grad<float>(g[i], count[i]); }
void pc_mean_grad_f64(const double* g, const int32_t* count, int n, double* out) { for (int i = 0; i < n; ++i) out[i] = pool_mean_grad<double>(g[i], count[i]); }

}
