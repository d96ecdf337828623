// Per-point arithmetic of the voxel-grid downsample (dicp_amd/voxel.py, csrc/voxel.hip).
//
// Plain inline C++, included by the HIP kernels and by a TEST-ONLY g++ build (tests/test_voxel_host.py) that holds these
// formulas to numpy on a CPU box with no GPU.
//
// For a row p of a cloud with origin o and voxel size s (both first converted to the points' dtype T):
//   v_d = floor((p_d - o_d) / s_d), in T: one rounded subtraction, one IEEE division (no reciprocal multiply), then floor;
//   a coordinate with |v_d| >= 2^62 (or not a number) is out of range and fails the call.
//   w_d = bit_length(max v_d - min v_d) over the cloud's rows; w_x + w_y + w_z > 64 fails the call.
//   key = (vx - min_x) << (w_y + w_z) | (vy - min_y) << w_z | (vz - min_z): ascending keys are ascending lexicographic (vx, vy, vz).
#pragma once
#include <math.h>
#include <stdint.h>

#include "dicp_math.h"

namespace dicp {

constexpr double VOX_COORD_LIMIT = 4611686018427387904.0;     // 2^62
constexpr int VOX_KEY_BITS = 64;

DICP_HD float  vox_floor(float x)  { return floorf(x); }
DICP_HD double vox_floor(double x) { return floor(x); }

// v = floor((p - o) / s) in T; false (and v = 0) when |v| >= 2^62 or v is not a number
template <typename T>
DICP_HD bool vox_coord(T p, T o, T s, int64_t* v) {
    const T d = p - o;
    const T q = d / s;
    const T f = vox_floor(q);
    const double fd = (double)f;                                // (exact for float and double)
    if (!(fd < VOX_COORD_LIMIT && fd > -VOX_COORD_LIMIT)) { *v = 0; return false; }
    *v = (int64_t)f;
    return true;
}

// bit_length(hi - lo) for lo <= hi inside (-2^62, 2^62): 0 for a single value
DICP_HD int vox_width(int64_t lo, int64_t hi) {
    const uint64_t r = (uint64_t)hi - (uint64_t)lo;
    return r ? 64 - __builtin_clzll(r) : 0;
}

DICP_HD bool vox_widths_ok(int wx, int wy, int wz) { return wx + wy + wz <= VOX_KEY_BITS; }

// 8-bit radix passes a cloud of these widths needs
DICP_HD int vox_passes(int wx, int wy, int wz) { return (wx + wy + wz + 7) / 8; }

DICP_HD uint64_t vox_shl(uint64_t x, int s) { return s >= 64 ? 0 : x << s; }

// v, lo: (3) voxel coordinates and the cloud's per-axis minimum; widths w_y, w_z
DICP_HD uint64_t vox_key(const int64_t* v, const int64_t* lo, int wy, int wz) {
    return vox_shl((uint64_t)v[0] - (uint64_t)lo[0], wy + wz) | vox_shl((uint64_t)v[1] - (uint64_t)lo[1], wz) | ((uint64_t)v[2] - (uint64_t)lo[2]);
}

}  // namespace dicp
