// Neighbourhood features (dicp_amd/group.py: group_points, interpolate_features, pool_neighbors), the per-slot rules of csrc/group.hip.
//
// Plain inline C++ templated on the scalar T, included by the HIP kernels and by TEST-ONLY g++ builds (tests/test_group_host.py,
// tests/test_pool_host.py) that run the same lines in a serial loop and hold them to the numpy restatements tests/group_ref.py, pool_ref.py.
//
// A slot (query i, slot s) names row idx[i, s] of a feature table of `rows` live rows.  It is LIVE when 0 <= idx < rows: one unsigned
// compare (a negative index is a huge unsigned one), so nothing is ever read out of range whatever idx holds.  Every other slot is empty:
// it gathers 0, takes no part in a sum and sends no gradient.
//   group:        out[i, s, c] = f[idx, c] (- centre[i, c] for c < Cc, one rounding)
//   interpolate:  a slot is live when its index is live and its d2 is finite.  r_s = 1 / (d2_s + eps), R = sum of r_s in slot order,
//                 w_s = r_s / R, out[c] = sum of w_s f[idx_s, c] in slot order (w * f + acc in one expression: it may fuse).
//                 d out[c] / d d2_s = -(r_s^2 / R) (f[idx_s, c] - out[c]).
//   pool:         over the live slots in slot order, per channel.  sum: acc = 0, acc = acc + f[idx_s, c] (plain additions: nothing to fuse).
//                 mean: the sum, then one division by T(count); 0 without a live slot.  max: the first live slot's value, replaced by a
//                 later v when v > best (ties keep the lowest slot; +0 and -0 tie) or when v is NaN and best is not (the first NaN stays);
//                 the argmax is the winning slot's ROW; 0 and -1 without a live slot.
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

// ------------------------------------------------------------------ pool
// one live slot's value v (of table row `row` >= 0) offered to the running maximum; arg < 0: no live slot yet
template <typename T>
DICP_HD void pool_max_step(T v, int row, T& best, int& arg) {
    if (arg < 0 || v > best || (v != v && best == best)) { best = v; arg = row; }
}
template <typename T>
DICP_HD T pool_sum_step(T acc, T v) { return acc + v; }
template <typename T>
DICP_HD T pool_mean(T sum, int count) { return count > 0 ? sum / T(count) : T(0); }
// what every live slot's row receives from the cotangent g of a mean over count > 0 slots
template <typename T>
DICP_HD T pool_mean_grad(T g, int count) { return g / T(count); }

}  // namespace dicp
