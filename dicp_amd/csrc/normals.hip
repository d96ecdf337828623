// Surface normals of point clouds (dicp_amd/normals.py): exact k nearest neighbours of every point within its own cloud,
// a covariance, its smallest eigenvector -- and the gradient of all that back to the points, for targets a network produces.
//
// Forward (dicp_normals_forward), all in the SORTED order of the existing sweep set-up:
//   pack     the xyz columns of (N,m,c) rows into (N,m,3)
//   sort     dicp_sweep_sort + dicp_sweep_build with frame = NULL: slot s of a cloud holds row tperm[s], ascending in raw x, the axes
//            as given -- so every distance below is the one the brute-force definition computes, bit for bit
//   walk     one lane per slot walks outward from its own slot with two cursors, the side with the smaller x gap first, and stops a
//            side once gap*gap > the k-th best d2 so far.  Exact: d2 = (xx + yy) + zz >= fl(dx*dx) = fl(gap*gap) for sums of
//            non-negative terms under round-to-nearest, and every row further out on that side has a larger gap.  Ties at the k-th
//            d2 are still examined, so the (d2, index) order holds.  The top-k list is a sorted register array, its insertion
//            unrolled (list and walk: csrc/dicp_topk.h); the block's slots +- WALK_HALO rows are staged in LDS.
//   normals  one lane per slot: the two-pass covariance of its neighbours, svd3, orientation, curvature (csrc/dicp_normals.h).
// Backward (dicp_normals_backward): one lane per slot recomputes its eigen-system from the saved neighbour slots and adds
// (2/k_eff) G (q_j - mu) to each neighbour j: into an LDS window of the block's slots +- BWD_HALO rows with LDS atomics, outside
// it into the sorted gradient rows with global atomics; the window is then flushed as contiguous rows, and one
// dicp_permute_add_rows returns the rows to the original order.  Float atomics: not bit-reproducible from run to run.
//
// method="grid" (dicp_normals_grid_forward / dicp_normals_grid_backward) replaces pack, sort and walk; the fit and the backward are the
// same two kernels on another layout (template parameter GRID):
//   grid     the density grid of the cloud itself (gknn_grid_build, kernels_grid.h) straight from the (N,m,c) rows: plans, keys, perm,
//            rows4, P = ball_slots(m) slots per cloud.  The live rows (j < rows[b], three finite coordinates) are slots 0 .. cnt - 1 in
//            (cell key, index) order, the other rows of the cloud slots cnt .. m - 1 in index order.
//   search   one lane per slot: gknn_scan (csrc/dicp_gridknn.h) of the slot's own row over the grid, the list of the walk.  The list is
//            the first k_eff(i) = min(k, #rows with a finite d2 to i) rows in (d2, index) order -- on a cloud the walk defines (live rows
//            finite, no d2 overflow) the walk's list, entry for entry, so the fit, which sums in list order in double, returns its bits.
//   layout   row stride P instead of m_pad, rows4 / perm for tgs4 / tperm, live = s < the plan's cnt instead of s < rows[b], and
//            k_eff = the filled entries of the slot's list instead of min(k, rows[b]).
// The backward window is BLOCK + 2 * BwdHalo slots of the grid's order, (vx, vy, vz) cell-major.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_fill.h"
#include "dicp_normals.h"
#include "dicp_topk.h"
#include "kernels_grid.h"
#include "kernels_normals.h"

namespace {

constexpr int NRM_KCAP_MIN = 8;                         // no list below 8 (k >= 3): the walk kernels are not instantiated for capacities 1 and 4
template <typename T> struct WalkHalo;                  // LDS rows staged on either side of a block's slots: 36 KiB float4 / 40 KiB double4
template <> struct WalkHalo<float>  { static constexpr int v = 1024; };
template <> struct WalkHalo<double> { static constexpr int v = 512; };
template <typename T> struct BwdHalo;                   // gradient window rows on either side: 27 KiB float / 30 KiB double
template <> struct BwdHalo<float>  { static constexpr int v = 1024; };
template <> struct BwdHalo<double> { static constexpr int v = 512; };

// ------------------------------------------------------------------ pack
template <typename T>
__global__ __launch_bounds__(BLOCK) void normals_pack_kernel(const T* __restrict__ pts, int c, size_t rows_total, T* __restrict__ xyz) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= rows_total) return;
    const T* p = pts + i * c;
    T* o = xyz + i * 3;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
}

// ------------------------------------------------------------------ walk (the list and the two cursors: csrc/dicp_topk.h)
template <typename T, int K>
__global__ __launch_bounds__(BLOCK) void normals_knn_kernel(const typename V4<T>::type* __restrict__ tgs4, const int32_t* __restrict__ tperm,
                                                            const int32_t* __restrict__ rows, int N, int m, int m_pad, int k, int bpc,
                                                            int32_t* __restrict__ nbr_s, int64_t* __restrict__ nbr_out,
                                                            unsigned long long* __restrict__ walked) {
    using T4 = typename V4<T>::type;
    constexpr int H = WalkHalo<T>::v;
    __shared__ T4 win[BLOCK + 2 * H];
    int b, blk;
    if (!decode_block(bpc, N, b, blk)) return;
    const int mb = rows_of(rows, b, m);
    const int s0 = blk * BLOCK, s = s0 + threadIdx.x;
    const size_t base = (size_t)b * m_pad;
    if (s0 >= m) return;                                    // (block-uniform)
    const int wlo = max(s0 - H, 0), whi = min(s0 + BLOCK + H, mb);
    for (int r = threadIdx.x; r < whi - wlo; r += BLOCK) win[r] = tgs4[base + wlo + r];
    __syncthreads();
    const bool live = s < mb;
    unsigned long long steps = 0;
    if (live) {
        auto row = [&](int j) -> T4 { return (j >= wlo && j < whi) ? win[j - wlo] : tgs4[base + j]; };
        auto orig = [&](int j) -> int { return tperm[base + j]; };
        T d[K];
        int id[K], sl[K];
        topk_init(d, id, sl, k);
        const auto ins = topk_inserter(d, id, sl, orig);
        const T4 p = row(s);
        ins(topk_d2<T>(p, p), s);
        steps = topk_walk(d, p, s - 1, s + 1, mb, row, ins);
        const size_t q = base + s;
        const int orow = tperm[q];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            if (i < K - k) continue;
            const int o = i - (K - k);
            nbr_s[q * k + o] = sl[i];
            if (nbr_out) nbr_out[((size_t)b * m + orow) * k + o] = id[i];
        }
    } else if (s < m && nbr_out) {                          // the row s of the cloud's padding (original order)
        for (int o = 0; o < k; ++o) nbr_out[((size_t)b * m + s) * k + o] = -1;
    }
    if (walked) wave_add(walked + b, steps);          // diagnostics: rows walked, one atomic per wave
}

// ------------------------------------------------------------------ grid search (the scan and its proof: csrc/dicp_gridknn.h)
// One lane per sorted slot s < m of the cloud's own grid: the query is the slot's row, so the grid's order is the query order and the
// lanes of a wave sit in the same or adjacent cells (their key searches and row reads hit the same lines).  Slots cnt .. m - 1 hold the
// rows that take no part (pad rows, non-finite rows): -1 neighbours at their original row.
template <typename T, int K>
__global__ __launch_bounds__(BLOCK) void normals_grid_knn_kernel(const void* __restrict__ plans, const uint64_t* __restrict__ keys,
                                                                 const int32_t* __restrict__ perm, const typename V4<T>::type* __restrict__ rows4,
                                                                 int N, int m, int P, int k, int bpc, int32_t* __restrict__ nbr_s,
                                                                 int64_t* __restrict__ nbr_out, unsigned long long* __restrict__ visited,
                                                                 unsigned long long* __restrict__ passes) {
    using T4 = typename V4<T>::type;
    int b, blk;
    if (!decode_block(bpc, N, b, blk)) return;
    const int s = blk * BLOCK + threadIdx.x;
    unsigned long long steps = 0, boxes = 0;
    if (s < m) {
        const size_t base = (size_t)b * P;
        const int orow = min(max(perm[base + s], 0), m - 1);
        if (s < plan_of<T>(plans, b).cnt) {
            const BallPlan<T> pl = plan_of<T>(plans, b);
            const uint64_t* kb = keys + base;
            auto key = [&](int j) -> uint64_t { return kb[j]; };
            auto row = [&](int j) -> T4 { return rows4[base + j]; };
            auto orig = [&](int j) -> int { return perm[base + j]; };
            T d[K];
            int id[K], sl[K];
            topk_init(d, id, sl, k);
            const auto ins = topk_inserter(d, id, sl, orig);
            const T4 p = rows4[base + s];
            const GknnScan r = gknn_scan<T>(pl, d, p, key, row, ins);
            steps = r.visited;
            boxes = (unsigned long long)r.passes;
            const size_t q = base + s;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                if (i < K - k) continue;
                const int o = i - (K - k);
                nbr_s[q * k + o] = sl[i];
                if (nbr_out) nbr_out[((size_t)b * m + orow) * k + o] = id[i];
            }
        } else if (nbr_out) {
            for (int o = 0; o < k; ++o) nbr_out[((size_t)b * m + orow) * k + o] = -1;
        }
    }
    if (visited) wave_add(visited + b, steps);        // diagnostics: rows fed and boxes computed, one atomic per wave each
    if (passes) wave_add(passes + b, boxes);
}

// ------------------------------------------------------------------ the fit (the two layouts and the eigen-system: csrc/kernels_normals.h)
template <typename T, bool GRID>
__global__ __launch_bounds__(BLOCK) void normals_point_kernel(const typename V4<T>::type* __restrict__ tgs4, const int32_t* __restrict__ tperm,
                                                              const int32_t* __restrict__ rows, const void* __restrict__ plans, int N, int m, int m_pad,
                                                              int k, int bpc, const int32_t* __restrict__ nbr_s, const T* __restrict__ vp, int vp_stride,
                                                              T* __restrict__ nrm, T* __restrict__ curv) {
    int b, blk;
    if (!decode_block(bpc, N, b, blk)) return;
    const int mb = nrm_live_rows<T, GRID>(rows, plans, b, m);
    const int s = blk * BLOCK + threadIdx.x;
    if (s >= m) return;
    const size_t base = (size_t)b * m_pad;
    const bool live = s < mb;
    const int k_eff = live ? nrm_k_eff<GRID>(nbr_s + (base + s) * k, k, mb) : 0;
    // the rows that take no part: the walk's padding is row s itself (original order), the grid's slots cnt .. m - 1 hold their rows
    const size_t orow = (size_t)b * m + (GRID ? min(max(tperm[base + s], 0), m - 1) : (live ? tperm[base + s] : s));
    T n[3] = {T(0), T(0), T(0)};
    T cv = T(0);
    if (live && k_eff >= 3) {
        NrmPoint P;
        nrm_point<T>(tgs4 + base, nbr_s + (base + s) * k, k_eff, tgs4[base + s], vp ? vp + (size_t)b * vp_stride : nullptr, P);
        n[0] = (T)(P.s * P.v[0]); n[1] = (T)(P.s * P.v[1]); n[2] = (T)(P.s * P.v[2]);
        cv = (T)nrm_curvature(P.lam);
    }
    nrm[orow * 3] = n[0]; nrm[orow * 3 + 1] = n[1]; nrm[orow * 3 + 2] = n[2];
    if (curv) curv[orow] = cv;
}

// ------------------------------------------------------------------ backward
template <typename T, bool GRID>
__global__ __launch_bounds__(BLOCK) void normals_bwd_kernel(const typename V4<T>::type* __restrict__ tgs4, const int32_t* __restrict__ tperm,
                                                            const int32_t* __restrict__ rows, const void* __restrict__ plans, int N, int m, int m_pad,
                                                            int k, int bpc, const int32_t* __restrict__ nbr_s, const T* __restrict__ vp, int vp_stride,
                                                            const T* __restrict__ g_nrm, const T* __restrict__ g_curv, T* __restrict__ gs /* (N,m_pad,3) sorted */) {
    constexpr int H = BwdHalo<T>::v;
    __shared__ T acc[(BLOCK + 2 * H) * 3];
    int b, blk;
    if (!decode_block(bpc, N, b, blk)) return;
    const int mb = nrm_live_rows<T, GRID>(rows, plans, b, m);
    const int s0 = blk * BLOCK, s = s0 + threadIdx.x;
    if (s0 >= mb) return;                                   // (block-uniform)
    const size_t base = (size_t)b * m_pad;
    const int wlo = max(s0 - H, 0), whi = min(s0 + BLOCK + H, mb), wn = (whi - wlo) * 3;
    for (int e = threadIdx.x; e < wn; e += BLOCK) acc[e] = T(0);
    __syncthreads();
    const int k_eff = s < mb ? nrm_k_eff<GRID>(nbr_s + (base + s) * k, k, mb) : 0;
    if (s < mb && k_eff >= 3) {
        const size_t orow = (size_t)b * m + (GRID ? min(max(tperm[base + s], 0), m - 1) : tperm[base + s]);
        double gn[3] = {0.0, 0.0, 0.0};
        if (g_nrm) { gn[0] = (double)g_nrm[orow * 3]; gn[1] = (double)g_nrm[orow * 3 + 1]; gn[2] = (double)g_nrm[orow * 3 + 2]; }
        const double gk = g_curv ? (double)g_curv[orow] : 0.0;
        if (gn[0] != 0.0 || gn[1] != 0.0 || gn[2] != 0.0 || gk != 0.0) {
            const auto p = tgs4[base + s];
            const int32_t* nb = nbr_s + (base + s) * k;
            NrmPoint P;
            nrm_point<T>(tgs4 + base, nb, k_eff, p, vp ? vp + (size_t)b * vp_stride : nullptr, P);
            double G6[6];
            if (nrm_grad_cov(P.lam, P.v, P.s, gn, gk, NrmTau<T>::v, G6)) {
                for (int o = 0; o < k_eff; ++o) {
                    const int j = nb[o];
                    if (j < 0) continue;
                    const auto y = tgs4[base + j];
                    const double dd[3] = {((double)y.x - (double)p.x) - P.mu[0], ((double)y.y - (double)p.y) - P.mu[1], ((double)y.z - (double)p.z) - P.mu[2]};
                    double g[3];
                    nrm_point_grad(G6, dd, k_eff, g);
                    if (j >= wlo && j < whi) {
                        T* a = acc + (j - wlo) * 3;
                        atomicAdd(a, (T)g[0]); atomicAdd(a + 1, (T)g[1]); atomicAdd(a + 2, (T)g[2]);
                    } else {                                // outside the window: the sorted rows directly
                        T* a = gs + (base + j) * 3;
                        unsafeAtomicAdd(a, (T)g[0]); unsafeAtomicAdd(a + 1, (T)g[1]); unsafeAtomicAdd(a + 2, (T)g[2]);
                    }
                }
            }
        }
    }
    __syncthreads();
    T* out = gs + (base + wlo) * 3;                         // the window: contiguous rows, which neighbouring blocks' windows overlap
    for (int e = threadIdx.x; e < wn; e += BLOCK) {
        const T v = acc[e];
        if (v != T(0)) unsafeAtomicAdd(out + e, v);
    }
}

}  // namespace

size_t dicp_normals_workspace_bytes(int dtype, int N, int m, int k, int c, int backward) {
    if (nrm_check(dtype, N, m, k, 0) || c < 3) return 0;
    const size_t ts = elem_size(dtype);
    if (backward) return up256((size_t)N * dicp_padded_targets(m) * 3 * ts);
    return nrm_layout(dtype, N, m, k).total;
}

int dicp_normals_forward(int dtype, const void* pts, int c, const int32_t* rows, int N, int m, int k, const void* viewpoint, int vp_per_cloud,
                         void* normals, void* curvature, int64_t* neighbors, void* workspace, size_t workspace_bytes,
                         unsigned long long* walked, void* stream) {
    if (!pts || !normals || !workspace) return DICP_ERR_NULL;
    int rc = nrm_check(dtype, N, m, k, vp_per_cloud);
    if (rc) return rc;
    if (c < 3) return DICP_ERR_SHAPE;
    const NrmLayout L = nrm_layout(dtype, N, m, k);
    if (workspace_bytes < L.total) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(pts, ts) || misaligned(normals, ts) || misaligned(curvature, ts) || misaligned(neighbors, 8) ||
        misaligned(viewpoint, ts)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int m_pad = dicp_padded_targets(m);
    void* xyz = ws + L.xyz;
    int32_t* tperm = (int32_t*)(ws + L.tperm);
    int32_t* nbr_s = (int32_t*)(ws + L.nbr_s);
    if (walked && (rc = dicp_fill::zero(walked, (size_t)N * sizeof(unsigned long long), st))) return rc;
    const size_t rows_total = (size_t)N * m;
    const unsigned gp = (unsigned)((rows_total + BLOCK - 1) / BLOCK);
    begin_launch();
    if (dtype == DICP_F32) normals_pack_kernel<float><<<gp, BLOCK, 0, st>>>((const float*)pts, c, rows_total, (float*)xyz);
    else                   normals_pack_kernel<double><<<gp, BLOCK, 0, st>>>((const double*)pts, c, rows_total, (double*)xyz);
    if ((rc = launch_status())) return rc;
    rc = dicp_sweep_sort(dtype, xyz, 3, nullptr, rows, N, m, m_pad, ws + L.keys, tperm, 0, nullptr, nullptr,
                         L.scratch_bytes ? ws + L.scratch : nullptr, L.scratch_bytes, stream);
    if (!rc) rc = dicp_sweep_build(dtype, xyz, 3, nullptr, rows, tperm, N, m, m_pad, ws + L.tgs4, nullptr, 0, stream);
    if (rc) return rc;
    const int bpc = (m_pad + BLOCK - 1) / BLOCK;
    const unsigned g = grid_for(N, bpc);
    const int vs = vp_per_cloud ? 3 : 0;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        const auto* tgs4 = (const typename V4<T>::type*)(ws + L.tgs4);
        topk_with_kcap(k < NRM_KCAP_MIN ? NRM_KCAP_MIN : k, [&](auto kcap) {
            constexpr int K = decltype(kcap)::value;
            if constexpr (K >= NRM_KCAP_MIN) normals_knn_kernel<T, K><<<g, BLOCK, 0, st>>>(tgs4, tperm, rows, N, m, m_pad, k, bpc, nbr_s, neighbors, walked);
        });
        normals_point_kernel<T, false><<<g, BLOCK, 0, st>>>(tgs4, tperm, rows, nullptr, N, m, m_pad, k, bpc, nbr_s, (const T*)viewpoint, vs, (T*)normals, (T*)curvature);
    });
    return launch_status();
}

int dicp_normals_backward(int dtype, const void* g_normals, const void* g_curvature, const void* viewpoint, int vp_per_cloud, const int32_t* rows,
                          int N, int m, int k, int c, const void* fwd_workspace, void* grad_pts, void* workspace, size_t workspace_bytes, void* stream) {
    if (!fwd_workspace || !grad_pts || !workspace) return DICP_ERR_NULL;
    int rc = nrm_check(dtype, N, m, k, vp_per_cloud);
    if (rc) return rc;
    if (c < 3 || workspace_bytes < dicp_normals_workspace_bytes(dtype, N, m, k, c, 1)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(fwd_workspace, 256) || misaligned(workspace, 16) || misaligned(grad_pts, ts) || misaligned(g_normals, ts) || misaligned(g_curvature, ts) ||
        misaligned(viewpoint, ts)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const NrmLayout L = nrm_layout(dtype, N, m, k);
    const char* ws = (const char*)fwd_workspace;
    const int m_pad = dicp_padded_targets(m);
    const int32_t* tperm = (const int32_t*)(ws + L.tperm);
    const size_t gs_bytes = (size_t)N * m_pad * 3 * ts;
    if ((rc = dicp_fill::zero(workspace, gs_bytes, st))) return rc;
    if ((rc = dicp_fill::zero(grad_pts, (size_t)N * m * c * ts, st))) return rc;
    if (!g_normals && !g_curvature) return 0;
    const int bpc = (m_pad + BLOCK - 1) / BLOCK;
    const unsigned g = grid_for(N, bpc);
    const int vs = vp_per_cloud ? 3 : 0;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        normals_bwd_kernel<T, false><<<g, BLOCK, 0, st>>>((const typename V4<T>::type*)(ws + L.tgs4), tperm, rows, nullptr, N, m, m_pad, k, bpc,
            (const int32_t*)(ws + L.nbr_s), (const T*)viewpoint, vs, (const T*)g_normals, (const T*)g_curvature, (T*)workspace);
    });
    if ((rc = launch_status())) return rc;
    return dicp_permute_add_rows(dtype, workspace, tperm, N, m_pad, m_pad, m_pad, 3, 3, grad_pts, m, c, stream);
}

size_t dicp_normals_grid_workspace_bytes(int dtype, int N, int m, int k, int c, int backward) {
    if (nrm_grid_check(dtype, N, m, k, c, 0)) return 0;
    const size_t ts = elem_size(dtype);
    if (backward) return up256((size_t)N * ball_slots(m) * 3 * ts);
    return nrm_grid_layout(dtype, N, m, k).total;
}

int dicp_normals_grid_forward(int dtype, const void* pts, int c, const int32_t* rows, int N, int m, int k, const void* viewpoint, int vp_per_cloud,
                              void* normals, void* curvature, int64_t* neighbors, void* workspace, size_t workspace_bytes,
                              unsigned long long* visited, unsigned long long* passes, void* stream) {
    if (!pts || !normals || !workspace) return DICP_ERR_NULL;
    int rc = nrm_grid_check(dtype, N, m, k, c, vp_per_cloud);
    if (rc) return rc;
    const NrmGridLayout L = nrm_grid_layout(dtype, N, m, k);
    if (workspace_bytes < L.total) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(pts, ts) || misaligned(rows, 4) || misaligned(normals, ts) || misaligned(curvature, ts) ||
        misaligned(neighbors, 8) || misaligned(viewpoint, ts) || misaligned(visited, 8) || misaligned(passes, 8)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    void* plans = ws + L.plans;
    uint64_t* keys = (uint64_t*)(ws + L.keys);
    int32_t* perm = (int32_t*)(ws + L.perm);
    int32_t* nbr_s = (int32_t*)(ws + L.nbr_s);
    if (visited && (rc = dicp_fill::zero(visited, (size_t)N * sizeof(unsigned long long), st))) return rc;
    if (passes && (rc = dicp_fill::zero(passes, (size_t)N * sizeof(unsigned long long), st))) return rc;
    const int P = ball_slots(m);
    const int bpc = (m + BLOCK - 1) / BLOCK;
    const unsigned g = grid_for(N, bpc);
    const int vs = vp_per_cloud ? 3 : 0;
    begin_launch();
    rc = with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        const auto* rows4 = (const typename V4<T>::type*)(ws + L.rows4);
        if (const int e = gknn_grid_build<T>((const T*)pts, c, rows, N, m, plans, keys, perm, ws + L.rows4, st)) return e;
        topk_with_kcap(k < NRM_KCAP_MIN ? NRM_KCAP_MIN : k, [&](auto kcap) {
            constexpr int K = decltype(kcap)::value;
            if constexpr (K >= NRM_KCAP_MIN) normals_grid_knn_kernel<T, K><<<g, BLOCK, 0, st>>>(plans, keys, perm, rows4, N, m, P, k, bpc, nbr_s, neighbors, visited, passes);
        });
        normals_point_kernel<T, true><<<g, BLOCK, 0, st>>>(rows4, perm, nullptr, plans, N, m, P, k, bpc, nbr_s, (const T*)viewpoint, vs, (T*)normals, (T*)curvature);
        return 0;
    });
    if (rc) return rc;
    return launch_status();
}

int dicp_normals_grid_backward(int dtype, const void* g_normals, const void* g_curvature, const void* viewpoint, int vp_per_cloud,
                               int N, int m, int k, int c, const void* fwd_workspace, void* grad_pts, void* workspace, size_t workspace_bytes, void* stream) {
    if (!fwd_workspace || !grad_pts || !workspace) return DICP_ERR_NULL;
    int rc = nrm_grid_check(dtype, N, m, k, c, vp_per_cloud);
    if (rc) return rc;
    if (workspace_bytes < dicp_normals_grid_workspace_bytes(dtype, N, m, k, c, 1)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(fwd_workspace, 256) || misaligned(workspace, 16) || misaligned(grad_pts, ts) || misaligned(g_normals, ts) || misaligned(g_curvature, ts) ||
        misaligned(viewpoint, ts)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const NrmGridLayout L = nrm_grid_layout(dtype, N, m, k);
    const char* ws = (const char*)fwd_workspace;
    const int P = ball_slots(m);
    const int32_t* perm = (const int32_t*)(ws + L.perm);
    if ((rc = dicp_fill::zero(workspace, (size_t)N * P * 3 * ts, st))) return rc;
    if ((rc = dicp_fill::zero(grad_pts, (size_t)N * m * c * ts, st))) return rc;
    if (!g_normals && !g_curvature) return 0;
    const int bpc = (m + BLOCK - 1) / BLOCK;
    const unsigned g = grid_for(N, bpc);
    const int vs = vp_per_cloud ? 3 : 0;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        normals_bwd_kernel<T, true><<<g, BLOCK, 0, st>>>((const typename V4<T>::type*)(ws + L.rows4), perm, nullptr, ws + L.plans, N, m, P, k, bpc,
            (const int32_t*)(ws + L.nbr_s), (const T*)viewpoint, vs, (const T*)g_normals, (const T*)g_curvature, (T*)workspace);
    });
    if ((rc = launch_status())) return rc;
    return dicp_permute_add_rows(dtype, workspace, perm, N, m, P, P, 3, 3, grad_pts, m, c, stream);   // (slots 0 .. m - 1 hold the cloud's m rows)
}
