// ISS keypoints for batches of clouds (dicp_amd/iss.py).  The rules are csrc/dicp_iss.h; everything is computed in double with no float
// atomics and nothing read back, so both passes are bit-reproducible and equal tests/iss_ref.py bit for bit.
//
// Both passes take one lane per row and one wave per workgroup: the wave reads the 64 k slots of its rows coalesced, resolves them
// (iss_neighbour) and transposes them through LDS with a leading dimension of 65 words, so that the write (consecutive lanes, consecutive
// slots) and the read (consecutive lanes, consecutive rows) are both free of bank conflicts.  Everything after that is lane-local.
// Pass 1 (dicp_iss_saliency): a lane walks its row's slots twice -- the sum of the mean and a 32-bit member mask, then the six sums of
//   the covariance over the members (the neighbour is gathered again: it is in the cache, and k x 3 doubles would not fit in registers) --
//   and runs the Jacobi sweeps: at most 18 rotations of two roots and three divisions each.  The double saliency goes to the workspace
//   (8 bytes per row, every row of the batch), the rounded outputs to the caller's tensors where asked for.
// Pass 2 (dicp_iss_maxima): per member one gathered point and one gathered 8-byte saliency, two compares.
// What bounds them (scripts/iss_bench.py, profiles/r31_iss_bench.txt; from the times alone, no counters): the gathers.  Both passes issue
//   2 k dependent gathers of 8- to 24-byte rows per lane and take about the same time, linear in k (pass 1: 0.036 ms per slot at 256 x
//   16384 rows); the Jacobi with its double divisions and roots is the part of pass 1 that does not depend on k, 0.12 of 1.28 ms at
//   k = 32.  Both stand at 2.6-3.7 x the time their bytes (idx once, 8 per slot; k gathered rows; the outputs) would need at 8 TB/s.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_iss.h"
#include "dicp_group_launch.h"

namespace {

constexpr int NB_LD = WAVE + 1;                     // leading dimension of the transposed slots in LDS: no bank conflicts either way
static_assert(ISS_K_MAX == GROUP_K_MAX && ISS_K_MAX <= 32, "the slots are those of the neighbour operators; the member mask has 32 bits");

template <typename T>
__device__ __forceinline__ void load3(const T* __restrict__ p, double* v) {
    v[0] = (double)p[0]; v[1] = (double)p[1]; v[2] = (double)p[2];
}

// the wave's slots, resolved and transposed: nb[s * NB_LD + r] = the row that slot s of row i0 + r names, or -1
template <typename I>
__device__ __forceinline__ void load_slots(const I* __restrict__ src, int nr, int k, int i0, int mb, int* nb) {
    for (int e = threadIdx.x; e < nr * k; e += WAVE) {
        const int r = e / k, s = e - r * k;
        nb[s * NB_LD + r] = iss_neighbour(src[e], i0 + r, mb);
    }
    __syncthreads();
}

// ------------------------------------------------------------------ pass 1
template <typename T, typename I>
__global__ __launch_bounds__(WAVE) void iss_saliency_kernel(const T* __restrict__ pts, int c, const I* __restrict__ idx, const int32_t* __restrict__ rows,
                                                            int m, int k, int bpc, double radius2, double gamma21, double gamma32, int min_neighbors,
                                                            double* __restrict__ sal_ws, T* __restrict__ sal_out, T* __restrict__ eig_out,
                                                            int32_t* __restrict__ count_out) {
    __shared__ int nb[NB_LD * ISS_K_MAX];
    const int b = blockIdx.x / bpc, i0 = (blockIdx.x - b * bpc) * WAVE;
    const int nr = min(WAVE, m - i0);                                   // >= 1: bpc = ceil(m / WAVE)
    const int mb = rows_of(rows, b, m);
    const size_t base = (size_t)b * m;
    const int lane = threadIdx.x;
    load_slots(idx + (base + i0) * k, nr, k, i0, mb, nb);
    if (lane >= nr) return;
    const int i = i0 + lane;
    double pi[3] = {0.0, 0.0, 0.0};
    bool ok_i = false;
    if (i < mb) {
        load3(pts + (base + i) * c, pi);
        ok_i = iss_row_ok(pi);
    }
    double l[3] = {0.0, 0.0, 0.0}, sal = 0.0;
    int count = 0;
    if (ok_i) {
        double sum[3] = {0.0, 0.0, 0.0};
        uint32_t members = 0u;
        count = 1;                                                      // the row itself: q = 0 adds nothing to the sum
        for (int s = 0; s < k; ++s) {
            const int j = nb[s * NB_LD + lane];                         // (j < mb <= m or -1)
            if (j < 0) continue;
            double pj[3], q[3];
            load3(pts + (base + j) * c, pj);
            const double r2 = iss_d2(pi, pj, q);
            if (!iss_member(iss_row_ok(pj), r2, radius2)) continue;
            members |= 1u << s;
            ++count;
            iss_mean_add(sum, q);
        }
        double mu[3], a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const double zero[3] = {0.0, 0.0, 0.0};
        iss_mean(sum, count, mu);
        iss_cov_add(a, zero, mu);
        for (int s = 0; s < k; ++s) {
            if (!((members >> s) & 1u)) continue;
            const int j = nb[s * NB_LD + lane];
            double pj[3], q[3];
            load3(pts + (base + j) * c, pj);
            iss_d2(pi, pj, q);
            iss_cov_add(a, q, mu);
        }
        iss_cov_scale(a, count);
        iss_eigenvalues(a, l);
        sal = iss_saliency(l, count, gamma21, gamma32, min_neighbors);
    }
    sal_ws[base + i] = sal;
    if (sal_out) sal_out[base + i] = (T)sal;
    if (eig_out) {
        T* e = eig_out + (base + i) * 3;
        e[0] = (T)l[0]; e[1] = (T)l[1]; e[2] = (T)l[2];
    }
    if (count_out) count_out[base + i] = count;
}

// ------------------------------------------------------------------ pass 2
template <typename T, typename I>
__global__ __launch_bounds__(WAVE) void iss_maxima_kernel(const T* __restrict__ pts, int c, const I* __restrict__ idx, const int32_t* __restrict__ rows,
                                                          int m, int k, int bpc, double radius2, int min_neighbors, const double* __restrict__ sal_ws,
                                                          uint8_t* __restrict__ mask) {
    __shared__ int nb[NB_LD * ISS_K_MAX];
    const int b = blockIdx.x / bpc, i0 = (blockIdx.x - b * bpc) * WAVE;
    const int nr = min(WAVE, m - i0);
    const int mb = rows_of(rows, b, m);
    const size_t base = (size_t)b * m;
    const int lane = threadIdx.x;
    load_slots(idx + (base + i0) * k, nr, k, i0, mb, nb);
    if (lane >= nr) return;
    const int i = i0 + lane;
    const double sal_i = sal_ws[base + i];                              // (pass 1 wrote every row i < m, 0 for pad and dead rows)
    bool keep = i < mb && sal_i > 0.0;                                  // (sal_i > 0: the row is OK)
    if (keep) {
        double pi[3];
        load3(pts + (base + i) * c, pi);
        int count = 1;
        for (int s = 0; s < k; ++s) {
            const int j = nb[s * NB_LD + lane];
            if (j < 0) continue;
            double pj[3], q[3];
            load3(pts + (base + j) * c, pj);
            const double r2 = iss_d2(pi, pj, q);
            if (!iss_member(iss_row_ok(pj), r2, radius2)) continue;
            ++count;
            if (iss_beats(sal_ws[base + j], j, sal_i, i)) keep = false;
        }
        keep = keep && count >= min_neighbors;
    }
    mask[base + i] = keep ? 1 : 0;
}

// ------------------------------------------------------------------ checks
inline int iss_blocks(int m) { return (m + WAVE - 1) / WAVE; }

int iss_shape(int N, int m) {
    if (N < 1 || m < 1) return DICP_ERR_SHAPE;
    if ((size_t)N * (size_t)m >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;          // fewer blocks than rows
    return 0;
}
int iss_check(int dtype, int idx64, int c, int N, int m, int k, double radius, int min_neighbors) {
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (idx64 != 0 && idx64 != 1) return DICP_ERR_ENUM;
    int rc = iss_shape(N, m);
    if (rc) return rc;
    if (c < 3 || k < ISS_K_MIN || k > ISS_K_MAX || min_neighbors < 1) return DICP_ERR_SHAPE;
    if (!fits62((size_t)N * m, (size_t)k, 8) || !fits62((size_t)N * m, (size_t)c, 8)) return DICP_ERR_SHAPE;
    if (!(radius == 0.0 || (radius > 0.0 && radius < HUGE_VAL))) return DICP_ERR_SHAPE;
    return 0;
}
inline bool bad_gamma(double g) { return !(g > 0.0 && g <= 1.0); }
inline size_t iss_ws_bytes(int N, int m) { return up256((size_t)N * m * sizeof(double)); }
// radius (0: none) -> radius2 of iss_member (< 0: none)
inline double iss_radius2(double radius) { return radius == 0.0 ? -1.0 : radius * radius; }

}  // namespace

size_t dicp_iss_workspace_bytes(int N, int m) {
    if (iss_shape(N, m)) return 0;
    return iss_ws_bytes(N, m);
}

int dicp_iss_saliency(int dtype, const void* points, int c, const void* idx, int idx64, const int32_t* rows, int N, int m, int k, double radius,
                      double gamma21, double gamma32, int min_neighbors, void* workspace, size_t workspace_bytes, void* saliency_out,
                      void* eigenvalues_out, int32_t* count_out, void* stream) {
    if (!points || !idx || !workspace) return DICP_ERR_NULL;
    int rc = iss_check(dtype, idx64, c, N, m, k, radius, min_neighbors);
    if (rc) return rc;
    if (bad_gamma(gamma21) || bad_gamma(gamma32)) return DICP_ERR_SHAPE;
    if (workspace_bytes < iss_ws_bytes(N, m)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(points, ts) || misaligned(saliency_out, ts) || misaligned(eigenvalues_out, ts)
        || misaligned(count_out, 4) || misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4))
        return DICP_ERR_ALIGN;
    const int bpc = iss_blocks(m);
    const unsigned g = (unsigned)N * (unsigned)bpc;
    const double radius2 = iss_radius2(radius);
    begin_launch();
    with_scalar_index(dtype, idx64, [&](auto t, auto i) {
        using T = decltype(t);
        using I = decltype(i);
        iss_saliency_kernel<T, I><<<g, WAVE, 0, (hipStream_t)stream>>>((const T*)points, c, (const I*)idx, rows, m, k, bpc, radius2, gamma21, gamma32,
                                                                       min_neighbors, (double*)workspace, (T*)saliency_out, (T*)eigenvalues_out, count_out);
    });
    return launch_status();
}

int dicp_iss_maxima(int dtype, const void* points, int c, const void* idx, int idx64, const int32_t* rows, int N, int m, int k, double radius,
                    int min_neighbors, const void* workspace, size_t workspace_bytes, uint8_t* mask_out, void* stream) {
    if (!points || !idx || !workspace || !mask_out) return DICP_ERR_NULL;
    int rc = iss_check(dtype, idx64, c, N, m, k, radius, min_neighbors);
    if (rc) return rc;
    if (workspace_bytes < iss_ws_bytes(N, m)) return DICP_ERR_SHAPE;
    if (misaligned(workspace, 256) || misaligned(points, elem_size(dtype)) || misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4))
        return DICP_ERR_ALIGN;
    const int bpc = iss_blocks(m);
    const unsigned g = (unsigned)N * (unsigned)bpc;
    const double radius2 = iss_radius2(radius);
    begin_launch();
    with_scalar_index(dtype, idx64, [&](auto t, auto i) {
        using T = decltype(t);
        using I = decltype(i);
        iss_maxima_kernel<T, I><<<g, WAVE, 0, (hipStream_t)stream>>>((const T*)points, c, (const I*)idx, rows, m, k, bpc, radius2, min_neighbors,
                                                                     (const double*)workspace, mask_out);
    });
    return launch_status();
}
