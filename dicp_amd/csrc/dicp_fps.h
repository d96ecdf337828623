// Farthest-point sampling (dicp_amd/fps.py), the per-row arithmetic and the comparison rule of csrc/fps.hip.
//
// Plain inline C++ templated on the scalar T, included by the HIP kernels and by a TEST-ONLY g++ build (tests/test_fps_host.py) that runs
// the same lines in a serial loop and holds them to a numpy restatement, index for index.
//
// A row's state is D: the minimum of d2 to the picks so far (+inf before the first), or the sentinel -1 for a row that can no longer be
// picked (already picked, past the cloud's row count, or with a non-finite coordinate).  d2(a, b) = (xx + yy) + zz with dx = b.x - a.x,
// xx = dx * dx, ... as separate statements (-ffp-contract=on fuses only inside one expression): the roundings numpy makes, and
// topk_d2's of dicp_topk.h.  A float32 overflow gives +inf, an ordinary value here.
// The next pick is the live row with the largest D, the lowest index among equals.  As a KEY that is one "larger wins" comparison:
// D >= 0 makes the bits of a float order-preserving as an unsigned integer, and ~index orders equal D by the lowest index.  float32 keys
// are one 64-bit word, (bits(D) << 32) | ~index; float64 keys are the pair (bits(D), ~index).  The all-zero key is "no live row": every
// real key has ~index >= 2^31.  Pick 0 uses the same key with 2^32 - 1 - rank in place of bits(D), rank = (index - start) mod rows.
#pragma once
#include <stdint.h>

#include "dicp_math.h"

namespace dicp {

template <typename T>
DICP_HD bool fps_finite(T x) { return x - x == T(0); }                 // false for inf and NaN

// a row that can be picked: inside the cloud's row count, x, y, z finite
template <typename T>
DICP_HD bool fps_candidate(int row, int rows, T x, T y, T z) { return row < rows && fps_finite(x) && fps_finite(y) && fps_finite(z); }

template <typename T>
DICP_HD T fps_d2(T ax, T ay, T az, T bx, T by, T bz) {
    const T dx = bx - ax;
    const T dy = by - ay;
    const T dz = bz - az;
    const T xx = dx * dx;
    const T yy = dy * dy;
    const T zz = dz * dz;
    const T s = xx + yy;
    return s + zz;
}

template <typename T>
DICP_HD T fps_picked() { return T(-1); }

// the row's D after a pick at distance d; a picked or non-candidate row stays at the sentinel
template <typename T>
DICP_HD T fps_update(T D, T d) { return (D >= T(0) && d < D) ? d : D; }

// the order of the picks: (Da, ia) goes before (Db, ib).  A thread's scan over its own rows uses this; across threads the same order is the key below
template <typename T>
DICP_HD bool fps_before(T Da, int ia, T Db, int ib) { return Da > Db || (Da == Db && ia < ib); }

// (index - start) mod rows for index, start mod rows in [0, rows)
DICP_HD uint32_t fps_rank(int row, int start, int rows) { return (uint32_t)(row >= start ? row - start : row - start + rows); }

template <typename T> struct FpsKey;
template <> struct FpsKey<float>  { uint64_t k; };
template <> struct FpsKey<double> { uint64_t hi; uint32_t lo; uint32_t pad; };

DICP_HD FpsKey<float> fps_key_none(float) { FpsKey<float> r; r.k = 0; return r; }
DICP_HD FpsKey<double> fps_key_none(double) { FpsKey<double> r; r.hi = 0; r.lo = 0; r.pad = 0; return r; }
DICP_HD FpsKey<float> fps_key(float D, int idx) {
    uint32_t b;
    __builtin_memcpy(&b, &D, 4);
    FpsKey<float> r;
    r.k = ((uint64_t)b << 32) | (uint32_t)~(uint32_t)idx;
    return r;
}
DICP_HD FpsKey<double> fps_key(double D, int idx) {
    FpsKey<double> r;
    __builtin_memcpy(&r.hi, &D, 8);
    r.lo = ~(uint32_t)idx;
    r.pad = 0;
    return r;
}
// the key of a live row (D >= 0), the empty key for the sentinel
template <typename T>
DICP_HD FpsKey<T> fps_key_live(T D, int idx) { return D >= T(0) ? fps_key(D, idx) : fps_key_none(T(0)); }
// pick 0: the smallest rank wins
DICP_HD FpsKey<float> fps_key_first(float, uint32_t rank, int idx) {
    FpsKey<float> r;
    r.k = ((uint64_t)(0xffffffffu - rank) << 32) | (uint32_t)~(uint32_t)idx;
    return r;
}
DICP_HD FpsKey<double> fps_key_first(double, uint32_t rank, int idx) {
    FpsKey<double> r;
    r.hi = 0xffffffffffffffffull - rank;
    r.lo = ~(uint32_t)idx;
    r.pad = 0;
    return r;
}
DICP_HD bool fps_key_empty(const FpsKey<float>& a) { return a.k == 0; }
DICP_HD bool fps_key_empty(const FpsKey<double>& a) { return a.hi == 0 && a.lo == 0; }
// a wins over b
DICP_HD bool fps_key_better(const FpsKey<float>& a, const FpsKey<float>& b) { return a.k > b.k; }
DICP_HD bool fps_key_better(const FpsKey<double>& a, const FpsKey<double>& b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }
DICP_HD int fps_key_index(const FpsKey<float>& a) { return (int)~(uint32_t)a.k; }
DICP_HD int fps_key_index(const FpsKey<double>& a) { return (int)~a.lo; }
DICP_HD float fps_key_D(const FpsKey<float>& a) {
    const uint32_t b = (uint32_t)(a.k >> 32);
    float D;
    __builtin_memcpy(&D, &b, 4);
    return D;
}
DICP_HD double fps_key_D(const FpsKey<double>& a) {
    double D;
    __builtin_memcpy(&D, &a.hi, 8);
    return D;
}

}  // namespace dicp
