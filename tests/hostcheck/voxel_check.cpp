// TEST-ONLY host build of dicp_amd/csrc/dicp_voxel.h (g++, no GPU): the per-point voxel arithmetic the HIP kernels execute,
// for tests/test_voxel_host.py.  Never loaded by dicp_amd.
#include "../../dicp_amd/csrc/dicp_voxel.h"

using namespace dicp;

extern "C" {

// v (n) and ok (n) for the points p (n) of one axis
void vc_coord_f32(const float* p, int n, float o, float s, int64_t* v, int32_t* ok) {
    for (int i = 0; i < n; ++i) ok[i] = vox_coord<float>(p[i], o, s, v + i) ? 1 : 0;
}
void vc_coord_f64(const double* p, int n, double o, double s, int64_t* v, int32_t* ok) {
    for (int i = 0; i < n; ++i) ok[i] = vox_coord<double>(p[i], o, s, v + i) ? 1 : 0;
}
int vc_width(int64_t lo, int64_t hi) { return vox_width(lo, hi); }
int vc_widths_ok(int wx, int wy, int wz) { return vox_widths_ok(wx, wy, wz) ? 1 : 0; }
int vc_passes(int wx, int wy, int wz) { return vox_passes(wx, wy, wz); }
// keys (n) of the coordinates v (n, 3) against the per-axis minimum lo (3)
void vc_keys(const int64_t* v, int n, const int64_t* lo, int wy, int wz, uint64_t* key) {
    for (int i = 0; i < n; ++i) key[i] = vox_key(v + 3 * i, lo, wy, wz);
}

}
