// TEST-ONLY host build of dicp_amd/csrc/dicp_normals_det.h (g++, no GPU): the deterministic gradient of the surface normals -- the list
// walk with its clamps and its entry check, the term from the query's record, the chunked sum -- that the HIP kernel executes, run in a
// serial loop over one cloud, for tests/test_normals_det_host.py.  Never loaded by dicp_amd.
#include <stdint.h>

#include "../../dicp_amd/csrc/dicp_normals_det.h"

using namespace dicp;

namespace {

template <typename T, typename I>
void det(const double* rec, const I* idx, int m, int k, int rows, int c, const int32_t* offsets, const int32_t* slots, T* out) {
    const NrmDetCloud<I> a = {rec, idx, m, k, rows < 0 ? 0 : (rows > m ? m : rows)};
    for (int j = 0; j < m; ++j) {
        T r[3];
        nrm_det_row<T, I>(a, offsets, slots, j, r);
        T* o = out + (size_t)j * c;
        o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
        for (int e = 3; e < c; ++e) o[e] = T(0);
    }
}

}  // namespace

extern "C" {

int nd_chunk() { return GROUP_DET_CHUNK; }
int nd_rec() { return NRM_REC; }

void nd_det_f32(const double* rec, const void* idx, int idx64, int m, int k, int rows, int c, const int32_t* offsets, const int32_t* slots, float* out) {
    if (idx64) det<float, int64_t>(rec, (const int64_t*)idx, m, k, rows, c, offsets, slots, out);
    else det<float, int32_t>(rec, (const int32_t*)idx, m, k, rows, c, offsets, slots, out);
}
void nd_det_f64(const double* rec, const void* idx, int idx64, int m, int k, int rows, int c, const int32_t* offsets, const int32_t* slots, double* out) {
    if (idx64) det<double, int64_t>(rec, (const int64_t*)idx, m, k, rows, c, offsets, slots, out);
    else det<double, int32_t>(rec, (const int32_t*)idx, m, k, rows, c, offsets, slots, out);
}

// a query's record as the records pass writes it
void nd_record(double* R, int on, const double* G6, const double* mu, const double* p, int k_eff) { nrm_det_record(R, on != 0, G6, mu, p, k_eff); }

}
