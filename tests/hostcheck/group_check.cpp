// TEST-ONLY host build of dicp_amd/csrc/dicp_group.h (g++, no GPU): liveness, the gather with its centre subtraction, the
// interpolation weights and the d2 gradient that the HIP kernels execute, run in a serial loop over one cloud, for tests/test_group_host.py.  Never loaded by dicp_amd.
#include <stdint.h>

#include "../../dicp_amd/csrc/dicp_group.h"

using namespace dicp;

namespace {

template <typename I>
void live(const I* idx, int rows, long long count, uint8_t* out) {
    for (long long i = 0; i < count; ++i) out[i] = group_row(idx[i], rows) >= 0;
}

template <typename T>
void group(const T* f, const int64_t* idx, int rows, const T* cen, int Cc, int n, int k, int C, T* out) {
    for (int i = 0; i < n; ++i)
        for (int s = 0; s < k; ++s) {
            const int j = group_row(idx[(size_t)i * k + s], rows);
            T* o = out + ((size_t)i * k + s) * C;
            for (int c = 0; c < C; ++c)
                o[c] = j >= 0 ? group_value<T>(f[(size_t)j * C + c], c < Cc ? cen[(size_t)i * Cc + c] : T(0), c < Cc) : T(0);
        }
}

// the slot's row (-1: empty index or non-finite d2) and r
template <typename T>
int slot(const int64_t* idx, const T* d2, T eps, size_t o, int rows, T& r) {
    int j = group_row(idx[o], rows);
    r = T(0);
    if (j >= 0) {
        if (group_finite(d2[o])) r = interp_r<T>(d2[o], eps); else j = -1;
    }
    return j;
}

template <typename T>
void interp(const T* f, const int64_t* idx, const T* d2, T eps, int rows, int n, int k, int C, T* out) {
    for (int i = 0; i < n; ++i) {
        T R = T(0), r;
        for (int s = 0; s < k; ++s) { slot<T>(idx, d2, eps, (size_t)i * k + s, rows, r); R = R + r; }
        for (int c = 0; c < C; ++c) {
            T acc = T(0);
            for (int s = 0; s < k; ++s) {
                const int j = slot<T>(idx, d2, eps, (size_t)i * k + s, rows, r);
                if (j >= 0) acc = interp_add<T>(acc, interp_w<T>(r, R), f[(size_t)j * C + c]);
            }
            out[(size_t)i * C + c] = acc;
        }
    }
}

template <typename T>
void interp_gd2_all(const T* f, const int64_t* idx, const T* d2, T eps, const T* g, const T* out, int rows, int n, int k, int C, T* gd2) {
    for (int i = 0; i < n; ++i) {
        T R = T(0), r;
        for (int s = 0; s < k; ++s) { slot<T>(idx, d2, eps, (size_t)i * k + s, rows, r); R = R + r; }
        for (int s = 0; s < k; ++s) {
            const int j = slot<T>(idx, d2, eps, (size_t)i * k + s, rows, r);
            T v = T(0);
            if (j >= 0) {
                T dot = T(0);
                for (int c = 0; c < C; ++c) dot = interp_dot_add<T>(dot, g[(size_t)i * C + c], f[(size_t)j * C + c], out[(size_t)i * C + c]);
                v = interp_gd2<T>(r, R, dot);
            }
            gd2[(size_t)i * k + s] = v;
        }
    }
}

}  // namespace

extern "C" {

void gc_live64(const int64_t* idx, int rows, long long count, uint8_t* out) { live<int64_t>(idx, rows, count, out); }
void gc_live32(const int32_t* idx, int rows, long long count, uint8_t* out) { live<int32_t>(idx, rows, count, out); }

#define GC_TYPE(T, S) \
    void gc_group_##S(const T* f, const int64_t* idx, int rows, const T* cen, int Cc, int n, int k, int C, T* out) { group<T>(f, idx, rows, cen, Cc, n, k, C, out); } \
    void gc_interp_##S(const T* f, const int64_t* idx, const T* d2, double eps, int rows, int n, int k, int C, T* out) { interp<T>(f, idx, d2, (T)eps, rows, n, k, C, out); } \
    void gc_gd2_##S(const T* f, const int64_t* idx, const T* d2, double eps, const T* g, const T* out, int rows, int n, int k, int C, T* gd2) { \
        interp_gd2_all<T>(f, idx, d2, (T)eps, g, out, rows, n, k, C, gd2); }
GC_TYPE(float, f32)
GC_TYPE(double, f64)

}
