// TEST-ONLY host build of dicp_amd/csrc/dicp_topk.h (g++, no GPU): the lower bound and the two-cursor walk the HIP kernels execute, driven the
// way csrc/knn_points.hip drives them (queries from another cloud), for tests/test_knn_points_host.py.  Never loaded by dicp_amd.
#include "../../dicp_amd/csrc/dicp_topk.h"

using namespace dicp;

template <typename T> struct Row3 { T x, y, z; };

// xs (n,3) queries; ys (m,3) the target rows sorted by x (NaN last), keys their x, perm their original indices.
// d2 / idx (n,k) out in query order; walked (n) the rows each query visited
template <typename T, int K>
static void run(const T* xs, int n, const T* ys, const T* keys, const int* perm, int m, int k, T* d2, long long* idx, unsigned* walked) {
    for (int i = 0; i < n; ++i) {
        const Row3<T> p{xs[3 * i], xs[3 * i + 1], xs[3 * i + 2]};
        const int pos = topk_lower_bound(keys, m, p.x);
        T d[K];
        int id[K], sl[K];
        topk_init(d, id, sl, k);
        auto row = [&](int j) { return Row3<T>{ys[3 * j], ys[3 * j + 1], ys[3 * j + 2]}; };
        auto orig = [&](int j) { return perm[j]; };
        const auto ins = topk_inserter(d, id, sl, orig);
        walked[i] = topk_walk(d, p, pos - 1, pos, m, row, ins);
        for (int o = 0; o < k; ++o) {
            d2[(long long)i * k + o] = d[K - k + o];
            idx[(long long)i * k + o] = id[K - k + o];
        }
    }
}

template <typename T>
static void dispatch(const T* xs, int n, const T* ys, const T* keys, const int* perm, int m, int k, T* d2, long long* idx, unsigned* walked) {
    if (k == 1) run<T, 1>(xs, n, ys, keys, perm, m, k, d2, idx, walked);
    else if (k <= 4) run<T, 4>(xs, n, ys, keys, perm, m, k, d2, idx, walked);
    else if (k <= 8) run<T, 8>(xs, n, ys, keys, perm, m, k, d2, idx, walked);
    else if (k <= 16) run<T, 16>(xs, n, ys, keys, perm, m, k, d2, idx, walked);
    else run<T, 32>(xs, n, ys, keys, perm, m, k, d2, idx, walked);
}

extern "C" {
void kc_knn_f32(const float* xs, int n, const float* ys, const float* keys, const int* perm, int m, int k, float* d2, long long* idx, unsigned* walked) {
    dispatch<float>(xs, n, ys, keys, perm, m, k, d2, idx, walked);
}
void kc_knn_f64(const double* xs, int n, const double* ys, const double* keys, const int* perm, int m, int k, double* d2, long long* idx, unsigned* walked) {
    dispatch<double>(xs, n, ys, keys, perm, m, k, d2, idx, walked);
}
}
