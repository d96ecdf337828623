// What a reader of a built cell grid needs of csrc/kernels_grid.h, without the kernels that build one: the slots of a cloud, its plan, the
// size check.  Shared by kernels_grid.h itself and by csrc/kernels_normals.h (csrc/normals_det.hip reads a grid and never builds one).
// Internal linkage, like dicp_common.h: each .hip file gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_ball.h"

namespace {

inline int ball_slots(int m) { int p = 2; while (p < m) p <<= 1; return p; }

template <typename T>
__device__ __forceinline__ const BallPlan<T>& plan_of(const void* plans, int b) {
    return *(const BallPlan<T>*)((const char*)plans + (size_t)b * BALL_PLAN_BYTES);
}

inline int ball_check(int dtype, int N, int m) {
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (N <= 0 || m <= 0 || m > (1 << 30)) return DICP_ERR_SHAPE;
    if ((size_t)N * ball_slots(m) > ((size_t)1 << 40)) return DICP_ERR_SHAPE;
    return 0;
}

}  // namespace
