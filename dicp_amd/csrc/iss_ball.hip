// Whole-ball ISS keypoints for batches of clouds (dicp_amd/iss.py: iss_saliency_ball / iss_keypoints_ball).  The rules are
// csrc/dicp_iss.h's, the member list, its order and the coverage proof of the walk csrc/dicp_iss_ball.h's; the grid is the one
// dicp_ball_grid_build makes (csrc/ball_query.hip), read here and never built.  No index and no d2 tensor is written or read: a lane
// walks its point's ball on the grid and accumulates while it walks.  Everything is in double with no float atomics and nothing read
// back: both passes are bit-reproducible and equal tests/iss_ball_ref.py bit for bit.
//
// Both passes take one lane per SORTED SLOT of the grid (P = 2^ceil(log2 m) per cloud), one wave per workgroup, so that the lanes of a
// wave are 64 consecutive rows of the cell order and walk the same cells; the outputs are scattered to the original row perm[slot].  The
// sort leaves the rows outside the grid (past rows[b], non-finite) and the padding indices m .. P - 1 behind the live rows, each once:
// a lane whose perm is below m stores its row's element of every output -- zeros / false for a row outside the grid --, the padding lanes
// store nothing.  So every element is stored exactly once and nothing is zero-filled.  The row's own coordinates come from rows4[slot]
// (one 16- / 32-byte load), as do the visited rows'.
// Pass 1 (dicp_iss_ball_saliency): walk 1 sums q and counts, then mu, walk 2 forms the six sums (the rows are read again: they are in
//   the cache, and a ball's rows do not fit in registers), then the Jacobi sweeps and the saliency; the double saliency goes to the
//   workspace (dicp_iss_workspace_bytes' layout: one double per original row), the rounded outputs where asked for.
// Pass 2 (dicp_iss_ball_maxima): one walk at the non-max radius; per member one gathered 4-byte perm and one gathered 8-byte saliency.  It
//   stops at the first member that beats the row: the mask is then false whatever the count is (dicp_iss_ball.h).
// What bounds them (scripts/iss_ball_bench.py, profiles/r35_iss_ball_bench.txt, 256 x 16384 rows; from the times and the visit counters,
//   no hardware counters): the rows VISITED, not the members, as expected before the bench ran.  With cells of edge R the range of a point
//   spans 3-4 cells per axis against a ball of 4.19 R^3: a walk visits 5.5-6 times the members on the uniform volume (351 rows for the two
//   walks of pass 1 at 29 members a ball, 2697 at 249) and 2.8 times on the planar scene, each visit one 16- / 32-byte load from L2 (the
//   lanes of a wave read the same lines), three subtractions, three products, two additions and a compare in double.  Pass 1 takes
//   4.2 / 9.4 / 20.3 ms at 29 / 89 / 249 members in float32 (4.6 / 10.5 / 23.6 in float64): 7.5-12 ns per point and visited row, falling
//   as the cells fill -- the binary search of every column (log2(cnt) dependent 8-byte key loads) and the Jacobi are the part that does
//   not grow with the ball.  350-560 G visited rows a second is 4-6 TFLOP/s of FP64, far below the vector rate: the walk is bound by its
//   dependent loads and by divergence (a wave runs as long as its slowest lane), not by arithmetic.  Pass 2 visits 41-146 rows a point
//   (it stops at the first member that beats the row) yet takes 2.6-7.8 ms: the rows that ARE maxima walk their whole range, and their
//   waves wait for them.
// `visited` (optional, for scripts/iss_ball_bench.py): the rows visited per cloud, added to the caller's zeroed counters with integer
//   atomics, one per lane -- a diagnostic that slows the pass down and touches no output.
// No spin-waits, no cooperative launch; every loop is bounded by the cloud's row count (iss_ball_scan's bound is ball_scan's).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_iss_ball.h"
#include "kernels_grid_plan.h"

namespace {

template <typename T>
__global__ __launch_bounds__(WAVE) void iss_ball_saliency_kernel(const void* __restrict__ plans, const uint64_t* __restrict__ keys,
                                                                 const int32_t* __restrict__ perm, const typename V4<T>::type* __restrict__ rows4,
                                                                 int m, int Pm, int bpc, double radius, double gamma21, double gamma32,
                                                                 int min_neighbors, double* __restrict__ sal_ws, T* __restrict__ sal_out,
                                                                 T* __restrict__ eig_out, int32_t* __restrict__ count_out,
                                                                 unsigned long long* __restrict__ visited_out) {
    using T4 = typename V4<T>::type;
    const int b = blockIdx.x / bpc, s = (blockIdx.x - b * bpc) * WAVE + threadIdx.x;
    if (s >= Pm) return;
    const size_t gbase = (size_t)b * Pm;
    const int i = perm[gbase + s];
    if (i < 0 || i >= m) return;                                        // the padding of the sort: no row of the outputs
    BallPlan<T> pl = plan_of<T>(plans, b);
    pl.cnt = min(max(pl.cnt, 0), m);                                    // (the grid's own count: the clamp is a belt for the loads below)
    double l[3] = {0.0, 0.0, 0.0}, sal = 0.0;
    int count = 0;
    if (s < pl.cnt) {                                                   // the live rows are the first cnt sorted slots
        const uint64_t* kb = keys + gbase;
        auto key = [&](int j) -> uint64_t { return kb[j]; };
        auto row = [&](int j) -> T4 { return rows4[gbase + j]; };
        unsigned visited;
        sal = iss_ball_saliency_row<T>(pl, iss_ball_R<T>(radius), radius * radius, s, key, row, gamma21, gamma32, min_neighbors, l, count, visited);
        if (visited_out) atomicAdd(visited_out + b, (unsigned long long)visited);            // diagnostics only: an integer count
    }
    const size_t o = (size_t)b * m + i;
    sal_ws[o] = sal;
    if (sal_out) sal_out[o] = (T)sal;
    if (eig_out) {
        T* e = eig_out + o * 3;
        e[0] = (T)l[0]; e[1] = (T)l[1]; e[2] = (T)l[2];
    }
    if (count_out) count_out[o] = count;
}

template <typename T>
__global__ __launch_bounds__(WAVE) void iss_ball_maxima_kernel(const void* __restrict__ plans, const uint64_t* __restrict__ keys,
                                                               const int32_t* __restrict__ perm, const typename V4<T>::type* __restrict__ rows4,
                                                               int m, int Pm, int bpc, double radius, int min_neighbors,
                                                               const double* __restrict__ sal_ws, uint8_t* __restrict__ mask,
                                                               unsigned long long* __restrict__ visited_out) {
    using T4 = typename V4<T>::type;
    const int b = blockIdx.x / bpc, s = (blockIdx.x - b * bpc) * WAVE + threadIdx.x;
    if (s >= Pm) return;
    const size_t gbase = (size_t)b * Pm, base = (size_t)b * m;
    const int i = perm[gbase + s];
    if (i < 0 || i >= m) return;
    BallPlan<T> pl = plan_of<T>(plans, b);
    pl.cnt = min(max(pl.cnt, 0), m);                                    // (the grid's own count: the clamp is a belt for the loads below)
    bool keep = false;
    if (s < pl.cnt) {
        const double sal_i = sal_ws[base + i];                          // (pass 1 wrote every row i < m)
        if (sal_i > 0.0) {
            const uint64_t* kb = keys + gbase;
            const int32_t* pb = perm + gbase;
            auto key = [&](int j) -> uint64_t { return kb[j]; };
            auto row = [&](int j) -> T4 { return rows4[gbase + j]; };
            auto orig = [&](int j) -> int { return min(max(pb[j], 0), m - 1); };      // (a live slot's row: the clamp is a belt)
            auto salj = [&](int j) -> double { return sal_ws[base + orig(j)]; };
            unsigned visited;
            keep = iss_ball_maximum_row<T>(pl, iss_ball_R<T>(radius), radius * radius, s, i, sal_i, min_neighbors, key, row, salj, orig, visited);
            if (visited_out) atomicAdd(visited_out + b, (unsigned long long)visited);
        }
    }
    mask[base + i] = keep ? 1 : 0;
}

// the checks of both entry points after the null checks, in the order that decides the status of a bad call
int iss_ball_check(int dtype, int N, int m, double radius, int min_neighbors, size_t workspace_bytes) {
    int rc = ball_check(dtype, N, m);
    if (rc) return rc;
    if ((size_t)N * (size_t)m >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;
    if ((size_t)N * (size_t)((ball_slots(m) + WAVE - 1) / WAVE) >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;
    if (min_neighbors < 1) return DICP_ERR_SHAPE;
    if (!(radius > 0.0 && radius < HUGE_VAL && radius * radius < HUGE_VAL)) return DICP_ERR_SHAPE;
    if (workspace_bytes < up256((size_t)N * m * sizeof(double))) return DICP_ERR_SHAPE;
    return 0;
}
inline bool bad_gamma(double g) { return !(g > 0.0 && g <= 1.0); }

}  // namespace

int dicp_iss_ball_saliency(int dtype, const void* plans, const uint64_t* keys, const int32_t* perm, const void* rows4, int N, int m, double radius,
                           double gamma21, double gamma32, int min_neighbors, void* workspace, size_t workspace_bytes, void* saliency_out,
                           void* eigenvalues_out, int32_t* count_out, unsigned long long* visited, void* stream) {
    if (!plans || !keys || !perm || !rows4 || !workspace) return DICP_ERR_NULL;
    int rc = iss_ball_check(dtype, N, m, radius, min_neighbors, workspace_bytes);
    if (rc) return rc;
    if (bad_gamma(gamma21) || bad_gamma(gamma32)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(plans, 8) || misaligned(keys, 8) || misaligned(perm, 4) || misaligned(rows4, 4 * ts) ||
        misaligned(saliency_out, ts) || misaligned(eigenvalues_out, ts) || misaligned(count_out, 4) || misaligned(visited, 8))
        return DICP_ERR_ALIGN;
    const int Pm = ball_slots(m), bpc = (Pm + WAVE - 1) / WAVE;
    const unsigned g = (unsigned)N * (unsigned)bpc;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        iss_ball_saliency_kernel<T><<<g, WAVE, 0, (hipStream_t)stream>>>(plans, keys, perm, (const typename V4<T>::type*)rows4, m, Pm, bpc, radius, gamma21,
                                                                         gamma32, min_neighbors, (double*)workspace, (T*)saliency_out, (T*)eigenvalues_out,
                                                                         count_out, visited);
    });
    return launch_status();
}

int dicp_iss_ball_maxima(int dtype, const void* plans, const uint64_t* keys, const int32_t* perm, const void* rows4, int N, int m, double radius,
                         int min_neighbors, const void* workspace, size_t workspace_bytes, uint8_t* mask_out, unsigned long long* visited,
                         void* stream) {
    if (!plans || !keys || !perm || !rows4 || !workspace || !mask_out) return DICP_ERR_NULL;
    int rc = iss_ball_check(dtype, N, m, radius, min_neighbors, workspace_bytes);
    if (rc) return rc;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(plans, 8) || misaligned(keys, 8) || misaligned(perm, 4) || misaligned(rows4, 4 * ts) ||
        misaligned(visited, 8))
        return DICP_ERR_ALIGN;
    const int Pm = ball_slots(m), bpc = (Pm + WAVE - 1) / WAVE;
    const unsigned g = (unsigned)N * (unsigned)bpc;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        iss_ball_maxima_kernel<T><<<g, WAVE, 0, (hipStream_t)stream>>>(plans, keys, perm, (const typename V4<T>::type*)rows4, m, Pm, bpc, radius,
                                                                       min_neighbors, (const double*)workspace, mask_out, visited);
    });
    return launch_status();
}
