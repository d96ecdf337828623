// TEST-ONLY host build of dicp_amd/csrc/dicp_knn_det.h (g++, no GPU): the deterministic y-gradient of the neighbour searches -- the list
// walk with its clamps and its entry check, the term, the chunked sum, in the serial form and in the hub form (the fold of the chunks'
// partials) -- that the HIP kernel executes, run in a serial loop over one cloud, for tests/test_knn_det_host.py.  Never loaded by dicp_amd.
#include <stdint.h>

#include "../../dicp_amd/csrc/dicp_knn_det.h"

using namespace dicp;

namespace {

// form 0: every list by the serial walk; 1: every list of more than one chunk by the hub fold; 2: the kernel's choice (KNN_DET_HUB)
template <typename T>
void det(int form, const T* g, const int64_t* idx, const T* x, int cx, int n, int k, const T* y, int cy, int m, int rows,
         const int32_t* offsets, const int32_t* slots, T* out) {
    const KnnDetCloud<T, int64_t> a = {g, idx, x, cx, n, k, rows};
    for (int l = 0; l < m; ++l) {
        T r[3] = {T(0), T(0), T(0)};
        if (l < rows) {
            int lo, hi;
            det_list(offsets, l, n * k, lo, hi);
            const T* yr = y + (size_t)l * cy;
            const bool hub = form == 1 ? hi - lo > GROUP_DET_CHUNK : (form == 2 && knn_det_is_hub(lo, hi));
            if (hub) knn_det_hub_sum<T, int64_t>(a, slots, l, yr, lo, hi, r);
            else knn_det_row_sum<T, int64_t>(a, slots, l, yr, lo, hi, r);
        }
        T* o = out + (size_t)l * cy;
        o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
        for (int c = 3; c < cy; ++c) o[c] = T(0);
    }
}

}  // namespace

extern "C" {

int kd_chunk() { return GROUP_DET_CHUNK; }
int kd_hub() { return KNN_DET_HUB; }

void kd_det_f32(int form, const float* g, const int64_t* idx, const float* x, int cx, int n, int k, const float* y, int cy, int m, int rows,
                const int32_t* offsets, const int32_t* slots, float* out) { det<float>(form, g, idx, x, cx, n, k, y, cy, m, rows, offsets, slots, out); }
void kd_det_f64(int form, const double* g, const int64_t* idx, const double* x, int cx, int n, int k, const double* y, int cy, int m, int rows,
                const int32_t* offsets, const int32_t* slots, double* out) { det<double>(form, g, idx, x, cx, n, k, y, cy, m, rows, offsets, slots, out); }

}
