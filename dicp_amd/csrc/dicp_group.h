// Neighbourhood features (dicp_amd/group.py: group_points, interpolate_features), the per-slot rules of csrc/group.hip.
//
// Plain inline C++ templated on the scalar T, included by the HIP kernels and by a TEST-ONLY g++ build (tests/test_group_host.py) that runs
// the same lines in a serial loop and holds them to the numpy restatement tests/group_ref.py.
//
// A slot (query i, slot s) names row idx[i, s] of a feature table of `rows` live rows.  It is LIVE when 0 <= idx < rows: one unsigned
// compare (a negative index is a huge unsigned one), so nothing is ever read out of range whatever idx holds.  Every other slot is empty:
// it gathers 0, takes no part in a sum and sends no gradient.
//   group:        out[i, s, c] = f[idx, c] (- centre[i, c] for c < Cc, one rounding)
//   interpolate:  a slot is live when its index is live and its d2 is finite.  r_s = 1 / (d2_s + eps), R = sum of r_s in slot order,
//                 w_s = r_s / R, out[c] = sum of w_s f[idx_s, c] in slot order (w * f + acc in one expression: it may fuse).
//                 d out[c] / d d2_s = -(r_s^2 / R) (f[idx_s, c] - out[c]).
#pragma once
#include <stdint.h>

#include "dicp_math.h"

namespace dicp {

constexpr int GROUP_K_MAX = 32;

// the row a slot names, or -1 for an empty slot.  rows in [0, 2^31)
DICP_HD int group_row(int64_t j, int rows) { return (uint64_t)j < (uint64_t)(uint32_t)rows ? (int)j : -1; }
DICP_HD int group_row(int32_t j, int rows) { return (uint32_t)j < (uint32_t)rows ? (int)j : -1; }

template <typename T>
DICP_HD bool group_finite(T x) { return x - x == T(0); }              // false for inf and NaN

// a gathered value of a live slot: column c of the row, the centre's column subtracted where there is one
template <typename T>
DICP_HD T group_value(T f, T centre, bool has_centre) { return has_centre ? f - centre : f; }

// ------------------------------------------------------------------ interpolate
template <typename T>
DICP_HD T interp_r(T d2, T eps) {
    const T s = d2 + eps;
    return T(1) / s;
}
template <typename T>
DICP_HD T interp_w(T r, T R) { return R > T(0) ? r / R : T(0); }
template <typename T>
DICP_HD T interp_add(T acc, T w, T f) { return w * f + acc; }
// one channel's share of the sum that g_d2 needs
template <typename T>
DICP_HD T interp_dot_add(T acc, T g, T f, T out) {
    const T d = f - out;
    return g * d + acc;
}
template <typename T>
DICP_HD T interp_gd2(T r, T R, T dot) {
    const T rr = r * r;
    const T q = rr / R;
    return -(q * dot);
}

}  // namespace dicp
