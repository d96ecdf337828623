// What the translation units of the neighbourhood-feature operators share (csrc/group.hip, csrc/inverse.hip): the 16-byte pack of the
// wide forms, the launch geometry of their grid-stride loops, the argument checks and the (scalar, index) type dispatch of their entry
// points.  Internal linkage, like dicp_common.h: each .hip file gets its own copy.  Include after dicp_common.h and dicp_group.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_group.h"

namespace {

constexpr unsigned GROUP_MAX_BLOCKS = 2048;         // 8 workgroups of 4 waves on each of 256 CUs: every wave slot of the chip

template <typename T, int V>
struct alignas(sizeof(T) * V) Pack { T v[V]; };

template <typename T, int V>
__device__ __forceinline__ Pack<T, V> pack_load(const T* p) { return *reinterpret_cast<const Pack<T, V>*>(p); }
template <typename T, int V>
__device__ __forceinline__ void pack_store(T* p, const Pack<T, V>& x) { *reinterpret_cast<Pack<T, V>*>(p) = x; }

inline unsigned group_grid(size_t items, int per_block) {
    const size_t g = (items + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : (g > GROUP_MAX_BLOCKS ? GROUP_MAX_BLOCKS : g));
}

// a * b * c < 2^62, without overflowing on the way (every factor >= 1 and < 2^31)
inline bool fits62(size_t a, size_t b, size_t c) {
    const size_t top = ((size_t)1 << 62) - 1;
    return a <= top / b && a * b <= top / c;
}

inline int group_check(int dtype, int idx64, int N, int n, int m, int k, int C) {
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (idx64 != 0 && idx64 != 1) return DICP_ERR_ENUM;
    if (N < 1 || n < 1 || m < 1 || k < 1 || k > GROUP_K_MAX || C < 1) return DICP_ERR_SHAPE;
    // the largest element count, N n k C of the grouped tensor, and the bytes of the gradient table, 8 N m C, stay below 2^62
    if (!fits62((size_t)N * n, (size_t)k, (size_t)C) || !fits62((size_t)N * m, 8, (size_t)C)) return DICP_ERR_SHAPE;
    return 0;
}
// rows of C elements are 16-byte segments from these bases on
inline bool vec16(int dtype, int C, const void* a, const void* b) { return ((size_t)C * elem_size(dtype)) % 16 == 0 && !(((uintptr_t)a | (uintptr_t)b) & 15); }

template <typename T> struct VecOf { static constexpr int v = 16 / sizeof(T); };

// f(T(), I()) for the scalar type T of the dtype and the index type I (idx64: int64_t, else int32_t)
template <typename F>
inline void with_scalar_index(int dtype, int idx64, F&& f) {
    with_scalar(dtype, [&](auto t) {
        if (idx64) f(t, int64_t());
        else f(t, int32_t());
    });
}

}  // namespace
