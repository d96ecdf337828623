// TEST-ONLY host build of dicp_amd/csrc/dicp_fps.h (g++, no GPU): the candidate test, d2, the update, the sentinel and the order of
// the picks that the HIP kernels execute, run in a serial loop over one cloud, for tests/test_fps_host.py.  Never loaded by dicp_amd.
#include <vector>

#include "../../dicp_amd/csrc/dicp_fps.h"

using namespace dicp;

namespace {

// use_key = 0: the order through fps_before; 1: through the packed keys the kernels reduce.  Returns k_eff
template <typename T>
int run(const T* pts, int c, int rows, long long start, int k, int use_key, int64_t* idx, T* dist) {
    const T inf = static_cast<T>(__builtin_huge_val());
    for (int t = 0; t < k; ++t) { idx[t] = -1; dist[t] = inf; }
    if (rows <= 0) return 0;
    std::vector<T> D(rows);
    const int st = (int)(start % rows);
    FpsKey<T> best = fps_key_none(T(0));
    for (int j = 0; j < rows; ++j) {
        const T* p = pts + (size_t)j * c;
        const bool cand = fps_candidate<T>(j, rows, p[0], p[1], p[2]);
        D[j] = cand ? inf : fps_picked<T>();
        if (cand) {
            const FpsKey<T> kr = fps_key_first(T(0), fps_rank(j, st, rows), j);
            if (fps_key_better(kr, best)) best = kr;
        }
    }
    if (fps_key_empty(best)) return 0;
    int pick = fps_key_index(best);
    for (int t = 0; t < k; ++t) {
        if (t > 0) {
            T bd = fps_picked<T>();
            int bj = -1;
            best = fps_key_none(T(0));
            for (int j = rows - 1; j >= 0; --j) {           // (descending: an order-dependent comparison would show)
                if (use_key) {
                    const FpsKey<T> kj = fps_key_live<T>(D[j], j);
                    if (fps_key_better(kj, best)) best = kj;
                } else if (D[j] >= T(0) && (bj < 0 || fps_before<T>(D[j], j, bd, bj))) {
                    bd = D[j]; bj = j;
                }
            }
            if (use_key) {
                if (fps_key_empty(best)) return t;
                bj = fps_key_index(best);
                bd = fps_key_D(best);
            }
            if (bj < 0) return t;
            pick = bj;
            dist[t] = bd;
        }
        idx[t] = pick;
        const T* q = pts + (size_t)pick * c;
        for (int j = 0; j < rows; ++j) {
            const T* p = pts + (size_t)j * c;
            D[j] = fps_update<T>(D[j], fps_d2<T>(p[0], p[1], p[2], q[0], q[1], q[2]));
        }
        D[pick] = fps_picked<T>();
    }
    return k;
}

}  // namespace

extern "C" {

int fc_run_f32(const float* pts, int c, int rows, long long start, int k, int use_key, int64_t* idx, float* dist) {
    return run<float>(pts, c, rows, start, k, use_key, idx, dist);
}
int fc_run_f64(const double* pts, int c, int rows, long long start, int k, int use_key, int64_t* idx, double* dist) {
    return run<double>(pts, c, rows, start, k, use_key, idx, dist);
}

}
