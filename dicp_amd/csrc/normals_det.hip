// The deterministic backward of the surface normals (estimate_normals with deterministic=True): two passes around the inverted index
// of the neighbour tensor (dicp_invert_neighbors).  The rules per element are csrc/dicp_normals_det.h's.
//
// The atomic backward (normals_bwd_kernel) gives every query a lane, which recomputes its eigen-system and scatters one term per
// neighbour with float atomics.  Here the two halves are separate kernels:
//   records  (dicp_normals_backward_records) one lane per sorted slot, as normals_bwd_kernel up to and including nrm_grad_cov (the same
//            nrm_point, nrm_k_eff, nrm_live_rows: csrc/kernels_normals.h): it writes, at the query's ORIGINAL row, the 13 doubles every
//            term of that query needs (G6, mu, p, f) and the query's neighbours as original rows (int32, -1 where none).  Rows that
//            take no part get an all-zero record and -1 neighbours, so both outputs are written in full.
//   gather   (dicp_normals_gather_det) one lane per original row j: y from its own record, then its list -- per entry the 4-byte
//            slot number, the index entry and the query's 104-byte record -- the term, the chunked sum; the row's c values stored once.
// No zero fill of the result, no float atomics, no permutation pass; nothing is read back.
//
// A lane per row and no wave-split for long lists: in a self-k-NN graph in 3-D the in-degree is bounded geometrically (a star layout
// reaches 105 at k = 16), and the longer lists of exact duplicates belong to queries that mostly carry no term
// (scripts/normals_det_bench.py measures a layout with duplicates).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_group.h"
#include "dicp_group_launch.h"
#include "dicp_inverse.h"
#include "dicp_normals_det.h"
#include "kernels_normals.h"

namespace {

// ------------------------------------------------------------------ records
template <typename T, bool GRID>
__global__ __launch_bounds__(BLOCK) void normals_records_kernel(const typename V4<T>::type* __restrict__ tgs4, const int32_t* __restrict__ tperm,
                                                                const int32_t* __restrict__ rows, const void* __restrict__ plans, int N, int m, int m_pad,
                                                                int k, int bpc, const int32_t* __restrict__ nbr_s, const T* __restrict__ vp, int vp_stride,
                                                                const T* __restrict__ g_nrm, const T* __restrict__ g_curv, double* __restrict__ records,
                                                                int32_t* __restrict__ nbr_o) {
    int b, blk;
    if (!decode_block(bpc, N, b, blk)) return;
    const int mb = nrm_live_rows<T, GRID>(rows, plans, b, m);
    const int s = blk * BLOCK + threadIdx.x;
    if (s >= m) return;
    const size_t base = (size_t)b * m_pad;
    const bool live = s < mb;
    // the rows that take no part: the walk's padding is row s itself (original order), the grid's slots cnt .. m - 1 hold their rows
    const size_t orow = (size_t)b * m + (size_t)min(max(GRID || live ? tperm[base + s] : s, 0), m - 1);
    const int32_t* nb = nbr_s + (base + s) * k;
    const int k_eff = live ? nrm_k_eff<GRID>(nb, k, mb) : 0;
    double R[NRM_REC];
#pragma unroll
    for (int e = 0; e < NRM_REC; ++e) R[e] = 0.0;
    if (live) {
        const auto p = tgs4[base + s];
        const double pd[3] = {(double)p.x, (double)p.y, (double)p.z};
        double G6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, mu[3] = {0.0, 0.0, 0.0};
        bool on = false;
        if (k_eff >= 3) {
            double gn[3] = {0.0, 0.0, 0.0};
            if (g_nrm) { gn[0] = (double)g_nrm[orow * 3]; gn[1] = (double)g_nrm[orow * 3 + 1]; gn[2] = (double)g_nrm[orow * 3 + 2]; }
            const double gk = g_curv ? (double)g_curv[orow] : 0.0;
            if (gn[0] != 0.0 || gn[1] != 0.0 || gn[2] != 0.0 || gk != 0.0) {
                NrmPoint P;
                nrm_point<T>(tgs4 + base, nb, k_eff, p, vp ? vp + (size_t)b * vp_stride : nullptr, P);
                on = nrm_grad_cov(P.lam, P.v, P.s, gn, gk, NrmTau<T>::v, G6);
                mu[0] = P.mu[0]; mu[1] = P.mu[1]; mu[2] = P.mu[2];
            }
        }
        nrm_det_record(R, on, G6, mu, pd, k_eff);
    }
    double* ro = records + orow * NRM_REC;
#pragma unroll
    for (int e = 0; e < NRM_REC; ++e) ro[e] = R[e];
    int32_t* no = nbr_o + orow * k;
    for (int o = 0; o < k; ++o) {
        const int j = live && o < k_eff ? nb[o] : -1;
        no[o] = j >= 0 && j < mb ? min(max(tperm[base + j], 0), m - 1) : -1;
    }
}

// ------------------------------------------------------------------ gather
template <typename T, typename I>
__global__ __launch_bounds__(BLOCK) void normals_gather_det_kernel(const double* __restrict__ records, const I* __restrict__ idx, const int32_t* __restrict__ rows,
                                                                   int m, int k, int c, const int32_t* __restrict__ offsets, const int32_t* __restrict__ slots,
                                                                   size_t total, T* __restrict__ grad_pts) {
    const size_t mk = (size_t)m * k;
    for (size_t row = (size_t)blockIdx.x * BLOCK + threadIdx.x; row < total; row += (size_t)gridDim.x * BLOCK) {
        const int b = (int)(row / m);
        const int j = (int)(row - (size_t)b * m);
        const NrmDetCloud<I> a = {records + (size_t)b * m * NRM_REC, idx + b * mk, m, k, rows_of(rows, b, m)};
        T out[3];
        nrm_det_row<T, I>(a, offsets + (size_t)b * ((size_t)m + 1), slots + b * mk, j, out);
        T* r = grad_pts + row * c;
        r[0] = out[0]; r[1] = out[1]; r[2] = out[2];
        for (int e = 3; e < c; ++e) r[e] = T(0);
    }
}

}  // namespace

int dicp_normals_backward_records(int dtype, int grid, const void* g_normals, const void* g_curvature, const void* viewpoint, int vp_per_cloud,
                                  const int32_t* rows, int N, int m, int k, int c, const void* fwd_workspace, size_t fwd_workspace_bytes,
                                  double* records, int32_t* nbr_o, void* stream) {
    if (!fwd_workspace || !records || !nbr_o) return DICP_ERR_NULL;
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (grid != 0 && grid != 1) return DICP_ERR_ENUM;
    int rc = grid ? nrm_grid_check(dtype, N, m, k, c, vp_per_cloud) : nrm_check(dtype, N, m, k, vp_per_cloud);
    if (rc) return rc;
    if (c < 3) return DICP_ERR_SHAPE;
    if (fwd_workspace_bytes < (grid ? nrm_grid_layout(dtype, N, m, k).total : nrm_layout(dtype, N, m, k).total)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(fwd_workspace, 256) || misaligned(records, 8) || misaligned(nbr_o, 4) || misaligned(g_normals, ts) || misaligned(g_curvature, ts) ||
        misaligned(viewpoint, ts) || misaligned(rows, 4)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const char* ws = (const char*)fwd_workspace;
    const int vs = vp_per_cloud ? 3 : 0;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        using T4 = typename V4<T>::type;
        if (grid) {
            const NrmGridLayout L = nrm_grid_layout(dtype, N, m, k);
            const int bpc = (m + BLOCK - 1) / BLOCK;
            normals_records_kernel<T, true><<<grid_for(N, bpc), BLOCK, 0, st>>>((const T4*)(ws + L.rows4), (const int32_t*)(ws + L.perm), nullptr, ws + L.plans, N, m,
                ball_slots(m), k, bpc, (const int32_t*)(ws + L.nbr_s), (const T*)viewpoint, vs, (const T*)g_normals, (const T*)g_curvature, records, nbr_o);
        } else {
            const NrmLayout L = nrm_layout(dtype, N, m, k);
            const int m_pad = dicp_padded_targets(m);
            const int bpc = (m_pad + BLOCK - 1) / BLOCK;
            normals_records_kernel<T, false><<<grid_for(N, bpc), BLOCK, 0, st>>>((const T4*)(ws + L.tgs4), (const int32_t*)(ws + L.tperm), rows, nullptr, N, m,
                m_pad, k, bpc, (const int32_t*)(ws + L.nbr_s), (const T*)viewpoint, vs, (const T*)g_normals, (const T*)g_curvature, records, nbr_o);
        }
    });
    return launch_status();
}

int dicp_normals_gather_det(int dtype, const double* records, const void* idx, int idx64, const int32_t* rows, int N, int m, int k, int c,
                            const int32_t* offsets, const int32_t* slots, void* grad_pts, void* stream) {
    if (!records || !idx || !offsets || !slots || !grad_pts) return DICP_ERR_NULL;
    int rc = group_check(dtype, idx64, N, m, m, k, c);
    if (rc) return rc;
    if (c < 3 || (size_t)m * k >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;             // a cloud's slot numbers are int32
    const size_t ts = elem_size(dtype);
    if (misaligned(records, 8) || misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4) || misaligned(offsets, 4) || misaligned(slots, 4) ||
        misaligned(grad_pts, ts)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const size_t total = (size_t)N * m;
    begin_launch();
    with_scalar_index(dtype, idx64, [&](auto t, auto i) {
        using T = decltype(t);
        using I = decltype(i);
        normals_gather_det_kernel<T, I><<<group_grid(total, BLOCK), BLOCK, 0, st>>>(records, (const I*)idx, rows, m, k, c, offsets, slots, total, (T*)grad_pts);
    });
    return launch_status();
}
