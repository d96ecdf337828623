// TEST-ONLY host build of dicp_amd/csrc/dicp_inverse.h (g++, no GPU): the sort key and the offsets rule of the inverted index, and the walk
// of the deterministic feature gradients -- the list's clamps, the entry check, the chunked sum, the first-of-query rule, every operator's
// term -- that the HIP kernels execute, run in a serial loop over one cloud, for tests/test_inverse_host.py.  Never loaded by dicp_amd.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../dicp_amd/csrc/dicp_inverse.h"

using namespace dicp;

namespace {

// the build as the kernels define it: keys, a stable sort of (key, q) fed in ascending q, payloads with -1 for empty slots, offsets from
// the sorted keys
template <typename I>
void invert(const I* idx, int rows, int n, int k, int m, int32_t* offsets, int32_t* slots) {
    const int64_t nk = (int64_t)n * k;
    std::vector<uint32_t> key(nk);
    std::vector<int32_t> order(nk);
    for (int64_t q = 0; q < nk; ++q) { key[q] = inverse_key(group_row(idx[q], rows), m); order[q] = (int32_t)q; }
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
    std::vector<uint32_t> sorted(nk);
    for (int64_t p = 0; p < nk; ++p) { sorted[p] = key[order[p]]; slots[p] = sorted[p] == (uint32_t)m ? -1 : order[p]; }
    for (int64_t p = 0; p <= nk; ++p) {
        int64_t first, last;
        inverse_offset_rows(sorted.data(), p, nk, m, first, last);
        for (int64_t j = first; j <= last; ++j) offsets[j] = (int32_t)p;
    }
}

template <typename T, typename I, int V>
void det_all(int op, const DetCloud<T, I>& a, const int32_t* offsets, const int32_t* slots, int m, T* out) {
    for (int j = 0; j < m; ++j)
        for (int c = 0; c < a.C; c += V) {
            T* o = out + (size_t)j * a.C + c;
            switch (op) {
            case DET_GROUP:     det_row_sum<T, I, V, DET_GROUP>(a, offsets, slots, j, c, o); break;
            case DET_POOL_SUM:  det_row_sum<T, I, V, DET_POOL_SUM>(a, offsets, slots, j, c, o); break;
            case DET_POOL_MEAN: det_row_sum<T, I, V, DET_POOL_MEAN>(a, offsets, slots, j, c, o); break;
            case DET_POOL_MAX:  det_row_sum<T, I, V, DET_POOL_MAX>(a, offsets, slots, j, c, o); break;
            default:            det_row_sum<T, I, V, DET_INTERP>(a, offsets, slots, j, c, o); break;
            }
        }
}

// packs: 1, or the 16-byte pack of the kernels' wide form (the caller passes aligned arrays and a C that is a multiple of it)
template <typename T, typename I>
void det(int op, int packs, const T* g, const I* idx, const int32_t* argmax, const int32_t* counts, const T* d2, double eps, int n, int k, int C, int rows, int m,
         const int32_t* offsets, const int32_t* slots, T* out) {
    const DetCloud<T, I> a = {g, idx, argmax, counts, d2, (T)eps, n, k, C, rows};
    if (packs == 1) det_all<T, I, 1>(op, a, offsets, slots, m, out);
    else det_all<T, I, 16 / sizeof(T)>(op, a, offsets, slots, m, out);
}

}  // namespace

extern "C" {

int ic_chunk() { return GROUP_DET_CHUNK; }
int ic_passes(int m) { return inverse_passes(m); }

#define IC_INDEX(I, W) \
    void ic_invert_##W(const I* idx, int rows, int n, int k, int m, int32_t* offsets, int32_t* slots) { invert<I>(idx, rows, n, k, m, offsets, slots); }
IC_INDEX(int64_t, i64)
IC_INDEX(int32_t, i32)

#define IC_TYPE(T, S, I, W) \
    void ic_det_##S##_##W(int op, int packs, const T* g, const I* idx, const int32_t* argmax, const int32_t* counts, const T* d2, double eps, int n, int k, int C, int rows, int m, \
                          const int32_t* offsets, const int32_t* slots, T* out) { \
        det<T, I>(op, packs, g, idx, argmax, counts, d2, eps, n, k, C, rows, m, offsets, slots, out); }
IC_TYPE(float, f32, int64_t, i64)
IC_TYPE(float, f32, int32_t, i32)
IC_TYPE(double, f64, int64_t, i64)
IC_TYPE(double, f64, int32_t, i32)

}
