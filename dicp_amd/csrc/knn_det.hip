// The deterministic y-gradient of the neighbour searches (dicp_knn_backward_y_det): knn_points with method="walk" and "grid", ball_query
// and both directions of chamfer_distance, with deterministic=True.  The rules per element are csrc/dicp_knn_det.h's.
//
// The atomic backwards (knn_points_bwd_kernel, ball_bwd_kernel) scatter one term per slot into grad_y; this is the gather over the
// inverted index of the PUBLIC idx output (dicp_invert_neighbors): knn_det_kernel gives every row of y one lane, which reads its row
// once, walks its list -- per entry the 4-byte cotangent and the 12-byte query row -- and stores the row's cy values once.  No zero
// fill, no float atomics, no workspace beyond the index; it reads the caller's x, y, g_d2 and idx, not the searches' sorted copies, so
// one entry point serves the three searches.
//
// Hubs.  Chamfer before alignment gives thousands of queries one nearest target, and a lane walking 16 384 gathered entries alone is a
// millisecond-scale tail.  After the lanes' own walks a wave therefore takes the rows whose lists are longer than KNN_DET_HUB chunks one
// at a time (lowest lane first; its l, lo, hi and coordinates are broadcast): lane c sums chunk c of a round of 64 chunks from +0, the
// round's partials are added in chunk order (by shuffle) to a total that every lane carries, and the owning lane stores the row.  The
// order of summation is the serial walk's (dicp_knn_det.h), so the same bits come out; no worklist, no second launch, nothing read back.
//
// KNN_DET_HUB = 4: the value with the lowest summed time of Chamfer's backward on the uniform and the hub layout among {2, 4, 8, 16}
// (scripts/knn_det_bench.py --sweep, profiles/r20_knn_det_bench.txt: 3.346, 3.317, 3.323 and 8.554 ms; the hub layout's lists are 16
// chunks and more, so 2, 4 and 8 differ by noise and 16 leaves them to single lanes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_group.h"
#include "dicp_group_launch.h"
#include "dicp_inverse.h"
#include "dicp_knn_det.h"

namespace {

template <typename T>
__global__ __launch_bounds__(BLOCK) void knn_det_kernel(const T* __restrict__ g_d2, const int64_t* __restrict__ idx, const int32_t* __restrict__ y_rows,
                                                        const T* __restrict__ x, int cx, int n, const T* __restrict__ y, int cy, int m, int k,
                                                        const int32_t* __restrict__ offsets, const int32_t* __restrict__ slots, size_t total,
                                                        T* __restrict__ grad_y) {
    const int lane = threadIdx.x & (WAVE - 1);
    const size_t nk = (size_t)n * k;
    const int nki = (int)nk;
    // (trips uniform over the workgroup: the wave's ballots and shuffles below need every lane)
    for (size_t base = (size_t)blockIdx.x * BLOCK; base < total; base += (size_t)gridDim.x * BLOCK) {
        const size_t row = base + threadIdx.x;
        const bool valid = row < total;
        int b = 0, l = 0, lo = 0, hi = 0;
        T yr[3] = {T(0), T(0), T(0)}, out[3] = {T(0), T(0), T(0)};
        bool hub = false;
        if (valid) {
            b = (int)(row / m);
            l = (int)(row - (size_t)b * m);
            const int rows = rows_of(y_rows, b, m);
            if (l < rows) {                                 // rows at or past the count: 0
                const T* yp = y + row * cy;
                yr[0] = yp[0]; yr[1] = yp[1]; yr[2] = yp[2];
                det_list(offsets + (size_t)b * ((size_t)m + 1), l, nki, lo, hi);
                hub = knn_det_is_hub(lo, hi);
                if (!hub) {
                    const KnnDetCloud<T, int64_t> a = {g_d2 + b * nk, idx + b * nk, x + (size_t)b * n * cx, cx, n, k, rows};
                    knn_det_row_sum<T, int64_t>(a, slots + b * nk, l, yr, lo, hi, out);
                }
            }
        }
        unsigned long long todo;
        while ((todo = __ballot(hub)) != 0ull) {
            const int src = __ffsll((long long)todo) - 1;
            const int hb = __shfl(b, src), hl = __shfl(l, src), hlo = __shfl(lo, src), hhi = __shfl(hi, src);
            const T hy[3] = {__shfl(yr[0], src), __shfl(yr[1], src), __shfl(yr[2], src)};
            const KnnDetCloud<T, int64_t> a = {g_d2 + hb * nk, idx + hb * nk, x + (size_t)hb * n * cx, cx, n, k, rows_of(y_rows, hb, m)};
            const int32_t* sl = slots + hb * nk;
            const int chunks = knn_det_chunks(hlo, hhi);
            T tot[3] = {T(0), T(0), T(0)};
            for (int c0 = 0; c0 < chunks; c0 += WAVE) {     // (chunks <= 2^31 / 64: c0 + WAVE does not overflow)
                T part[3] = {T(0), T(0), T(0)};
                if (c0 + lane < chunks) knn_det_chunk<T, int64_t>(a, sl, hl, hy, hlo, hhi, c0 + lane, part);
                const int cnt = min(WAVE, chunks - c0);
                for (int t = 0; t < cnt; ++t) {
#pragma unroll
                    for (int v = 0; v < 3; ++v) {
                        const T p = __shfl(part[v], t);
                        tot[v] = tot[v] + p;
                    }
                }
            }
            if (lane == src) {
                out[0] = tot[0]; out[1] = tot[1]; out[2] = tot[2];
                hub = false;
            }
        }
        if (valid) {
            T* r = grad_y + row * cy;
            r[0] = out[0]; r[1] = out[1]; r[2] = out[2];
            for (int c = 3; c < cy; ++c) r[c] = T(0);
        }
    }
}

}  // namespace

int dicp_knn_backward_y_det(int dtype, const void* g_d2, const int64_t* idx, const int32_t* y_rows, const void* x, int cx, int n,
                            const void* y, int cy, int m, int N, int k, const int32_t* offsets, const int32_t* slots, void* grad_y, void* stream) {
    if (!g_d2 || !idx || !x || !y || !offsets || !slots || !grad_y) return DICP_ERR_NULL;
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (N < 1 || n < 1 || m < 1 || k < 1 || k > GROUP_K_MAX || cx < 3 || cy < 3) return DICP_ERR_SHAPE;
    if ((size_t)n * k >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;                       // a cloud's slot numbers are int32
    // the element counts N n k, N n cx and the bytes of the gradient, 8 N m cy, stay below 2^62
    if (!fits62((size_t)N * n, (size_t)k, (size_t)cx) || !fits62((size_t)N * m, 8, (size_t)cy)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(g_d2, ts) || misaligned(x, ts) || misaligned(y, ts) || misaligned(grad_y, ts) || misaligned(idx, 8) || misaligned(y_rows, 4) ||
        misaligned(offsets, 4) || misaligned(slots, 4)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const size_t total = (size_t)N * m;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        knn_det_kernel<T><<<group_grid(total, BLOCK), BLOCK, 0, st>>>((const T*)g_d2, idx, y_rows, (const T*)x, cx, n, (const T*)y, cy, m, k, offsets, slots,
                                                                    total, (T*)grad_y);
    });
    return launch_status();
}
