// FPFH descriptors for batches of clouds (dicp_amd/fpfh.py).  The rules are csrc/dicp_fpfh.h; everything is computed in double with no
// float atomics, so both passes are bit-reproducible and equal tests/fpfh_ref.py bit for bit.
//
// Pass 1 (dicp_fpfh_spfh), one lane per (row, slot): a workgroup takes R = min(256 / k, 64) whole rows of one cloud, so its k R slots
//   of idx are one contiguous, coalesced read.  A lane gathers the neighbour's point and normal, computes the pair's three bins and adds 1
//   to three of its row's 33 counters in LDS (integer atomics: the counts do not depend on the order).  The workgroup then stores its rows
//   of the internal table -- FPFH_ROW_BYTES = 48 per row: the 33 counts as bytes, the number of pairs, the row's OK flag -- as 4-byte words,
//   coalesced, and the plain (N, m, 33) byte tensor if the caller asked for it.  Bound by the double arithmetic of the frame (two roots and
//   five divisions per pair) and the 2 x 3 gathered values per pair; idx is 4 or 8 bytes per pair.
// Pass 2 (dicp_fpfh_combine), one lane per row, one wave per workgroup: the wave reads the 64 k slots of its rows coalesced, resolves them
//   (fpfh_neighbour) and transposes them through LDS; a lane then walks its row's slots in order with the 33 sums in registers, and per near
//   slot gathers the neighbour's point and its 48-byte table row (three aligned 16-byte loads: s_j is formed on the fly, 33 divisions).
//   The 64 x 33 results go through LDS and are stored coalesced.  Bound by the 33 double divisions per (row, slot).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_fpfh.h"
#include "dicp_group_launch.h"

namespace {

constexpr int SPFH_ROWS = 64;                       // the most rows a workgroup of pass 1 takes
constexpr int ROW_WORDS = FPFH_ROW_BYTES / 4;
constexpr int NB_LD = WAVE + 1;                     // leading dimension of the transposed slots in LDS: no bank conflicts either way
static_assert(FPFH_ROW_BYTES % 16 == 0 && FPFH_ROW_OK < FPFH_ROW_BYTES && FPFH_K_MAX <= 255, "a table row is whole 16-byte words; a count is a byte");
static_assert(FPFH_K_MAX == GROUP_K_MAX, "the slots are those of the neighbour operators");

inline int spfh_rows_per_block(int k) { const int r = BLOCK / k; return r < SPFH_ROWS ? r : SPFH_ROWS; }

template <typename T>
__device__ __forceinline__ void load3(const T* __restrict__ p, double* v) {
    v[0] = (double)p[0]; v[1] = (double)p[1]; v[2] = (double)p[2];
}

// ------------------------------------------------------------------ pass 1
template <typename T, typename I>
__global__ __launch_bounds__(BLOCK) void fpfh_spfh_kernel(const T* __restrict__ pts, int c, const T* __restrict__ nrm, const I* __restrict__ idx,
                                                          const int32_t* __restrict__ rows, int m, int k, int R, int bpc, double radius2,
                                                          uint32_t* __restrict__ table, uint8_t* __restrict__ spfh) {
    __shared__ unsigned cnt[SPFH_ROWS * FPFH_CH];
    __shared__ unsigned okf[SPFH_ROWS];
    const int b = blockIdx.x / bpc, i0 = (blockIdx.x - b * bpc) * R;
    const int nr = min(R, m - i0);                                      // >= 1: bpc = ceil(m / R)
    const int mb = rows_of(rows, b, m);
    const size_t base = (size_t)b * m;
    for (int t = threadIdx.x; t < nr * FPFH_CH; t += BLOCK) cnt[t] = 0u;
    __syncthreads();
    const int r = threadIdx.x / k, s = threadIdx.x - r * k;
    if (r < nr) {
        const int i = i0 + r;
        double pi[3], ni[3];
        bool ok_i = false;
        if (i < mb) {
            load3(pts + (base + i) * c, pi);
            load3(nrm + (base + i) * 3, ni);
            ok_i = fpfh_row_ok(pi, ni);
        }
        if (s == 0) okf[r] = ok_i ? 1u : 0u;
        const int j = fpfh_neighbour(idx[(base + i) * k + s], i, mb);     // (the read is inside idx whatever it holds; j < mb <= m or -1)
        if (ok_i && j >= 0) {
            double pj[3], nj[3], d[3];
            load3(pts + (base + j) * c, pj);
            load3(nrm + (base + j) * 3, nj);
            const double r2 = fpfh_d2(pi, pj, d);
            int ch[3];
            if (fpfh_near(true, fpfh_row_ok(pj, nj), r2, radius2) && fpfh_pair_bins(ni, nj, d, r2, ch)) {
                atomicAdd(&cnt[r * FPFH_CH + ch[0]], 1u);
                atomicAdd(&cnt[r * FPFH_CH + ch[1]], 1u);
                atomicAdd(&cnt[r * FPFH_CH + ch[2]], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t* tb = table + (base + i0) * ROW_WORDS;
    for (int t = threadIdx.x; t < nr * ROW_WORDS; t += BLOCK) {
        const int rr = t / ROW_WORDS, w = t - rr * ROW_WORDS;
        const unsigned* cr = cnt + rr * FPFH_CH;
        uint32_t word = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int q = 4 * w + e;
            unsigned v = 0u;
            if (q < FPFH_CH) v = cr[q];
            else if (q == FPFH_ROW_C) { for (int a = 0; a < FPFH_BINS; ++a) v += cr[a]; }
            else if (q == FPFH_ROW_OK) v = okf[rr];
            word |= v << (8 * e);
        }
        tb[t] = word;
    }
    if (spfh) {
        uint8_t* sp = spfh + (base + i0) * FPFH_CH;
        for (int t = threadIdx.x; t < nr * FPFH_CH; t += BLOCK) sp[t] = (uint8_t)cnt[t];
    }
}

// ------------------------------------------------------------------ pass 2
__device__ __forceinline__ unsigned row_byte(const uint32_t* w, int q) { return (w[q >> 2] >> (8 * (q & 3))) & 0xffu; }
__device__ __forceinline__ void load_row(const uint4* __restrict__ table, size_t row, uint32_t* w) {
    const uint4* p = table + row * (FPFH_ROW_BYTES / 16);
#pragma unroll
    for (int a = 0; a < FPFH_ROW_BYTES / 16; ++a) {
        const uint4 v = p[a];
        w[4 * a] = v.x; w[4 * a + 1] = v.y; w[4 * a + 2] = v.z; w[4 * a + 3] = v.w;
    }
}

template <typename T, typename I>
__global__ __launch_bounds__(WAVE) void fpfh_combine_kernel(const T* __restrict__ pts, int c, const I* __restrict__ idx, const int32_t* __restrict__ rows,
                                                            int m, int k, int bpc, double radius2, const uint4* __restrict__ table, T* __restrict__ out) {
    __shared__ double lds_raw[WAVE * FPFH_CH];                          // the transposed slots (int), then the results (T)
    static_assert(sizeof(double) * WAVE * FPFH_CH >= sizeof(int) * NB_LD * FPFH_K_MAX, "the slots fit");
    int* nb = reinterpret_cast<int*>(lds_raw);
    T* res = reinterpret_cast<T*>(lds_raw);
    const int b = blockIdx.x / bpc, i0 = (blockIdx.x - b * bpc) * WAVE;
    const int nr = min(WAVE, m - i0);
    const int mb = rows_of(rows, b, m);
    const size_t base = (size_t)b * m;
    const int lane = threadIdx.x;
    {
        const I* src = idx + (base + i0) * k;
        for (int e = lane; e < nr * k; e += WAVE) {
            const int r = e / k, s = e - r * k;
            nb[s * NB_LD + r] = fpfh_neighbour(src[e], i0 + r, mb);
        }
    }
    __syncthreads();
    const int i = i0 + lane;
    const bool live = lane < nr;
    uint32_t wi[ROW_WORDS];
#pragma unroll
    for (int a = 0; a < ROW_WORDS; ++a) wi[a] = 0u;
    double pi[3] = {0.0, 0.0, 0.0};
    if (live) {                                                         // (pass 1 wrote every row i < m of the table, pad rows with zeros)
        load_row(table, base + i, wi);
        load3(pts + (base + i) * c, pi);
    }
    const bool ok_i = live && i < mb && row_byte(wi, FPFH_ROW_OK) != 0u;
    double acc[FPFH_CH];
#pragma unroll
    for (int ch = 0; ch < FPFH_CH; ++ch) acc[ch] = 0.0;
    for (int s = 0; s < k; ++s) {
        const int j = ok_i ? nb[s * NB_LD + lane] : -1;
        if (j < 0) continue;
        uint32_t wj[ROW_WORDS];
        double pj[3], d[3];
        load_row(table, base + j, wj);
        load3(pts + (base + j) * c, pj);
        const double r2 = fpfh_d2(pi, pj, d);
        if (!fpfh_near(true, row_byte(wj, FPFH_ROW_OK) != 0u, r2, radius2)) continue;
        const double wt = fpfh_weight(r2);
        const int cj = (int)row_byte(wj, FPFH_ROW_C);
#pragma unroll
        for (int ch = 0; ch < FPFH_CH; ++ch) acc[ch] = fpfh_weight_add(acc[ch], wt, fpfh_spfh((int)row_byte(wj, ch), cj));
    }
    __syncthreads();                                                    // (the slots have been read: the buffer now takes the results)
    if (live) {
        const int ci = (int)row_byte(wi, FPFH_ROW_C);
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            double S = 0.0;
#pragma unroll
            for (int a = 0; a < FPFH_BINS; ++a) S = S + acc[g * FPFH_BINS + a];
#pragma unroll
            for (int a = 0; a < FPFH_BINS; ++a) {
                const int ch = g * FPFH_BINS + a;
                res[lane * FPFH_CH + ch] = (T)fpfh_out(acc[ch], S, fpfh_spfh((int)row_byte(wi, ch), ci));
            }
        }
    }
    __syncthreads();
    T* dst = out + (base + i0) * FPFH_CH;
    for (int e = lane; e < nr * FPFH_CH; e += WAVE) dst[e] = res[e];
}

// ------------------------------------------------------------------ checks
inline int fpfh_blocks1(int m, int k) { const int R = spfh_rows_per_block(k); return (m + R - 1) / R; }
inline int fpfh_blocks2(int m) { return (m + WAVE - 1) / WAVE; }

int fpfh_shape(int N, int m) {
    if (N < 1 || m < 1) return DICP_ERR_SHAPE;
    if ((size_t)N * (size_t)m > (size_t)0x7fffffff) return DICP_ERR_SHAPE;          // one block per row at most (k = 1 ... : fewer)
    return 0;
}
int fpfh_check(int dtype, int idx64, int c, int N, int m, int k, double radius) {
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (idx64 != 0 && idx64 != 1) return DICP_ERR_ENUM;
    int rc = fpfh_shape(N, m);
    if (rc) return rc;
    if (c < 3 || k < FPFH_K_MIN || k > FPFH_K_MAX) return DICP_ERR_SHAPE;
    if (!fits62((size_t)N * m, (size_t)k, 8) || !fits62((size_t)N * m, (size_t)c, 8)) return DICP_ERR_SHAPE;
    if (!(radius == 0.0 || (radius > 0.0 && radius < HUGE_VAL))) return DICP_ERR_SHAPE;
    return 0;
}
inline size_t fpfh_table_bytes(int N, int m) { return up256((size_t)N * m * FPFH_ROW_BYTES); }
// radius (0: none) -> radius2 of fpfh_near (< 0: none).  A radius whose square underflows to 0 admits nothing: r2 > 0 and r2 <= 0 never hold together
inline double fpfh_radius2(double radius) { return radius == 0.0 ? -1.0 : radius * radius; }

}  // namespace

size_t dicp_fpfh_workspace_bytes(int N, int m) {
    if (fpfh_shape(N, m)) return 0;
    return fpfh_table_bytes(N, m);
}

int dicp_fpfh_spfh(int dtype, const void* points, int c, const void* normals, const void* idx, int idx64, const int32_t* rows, int N, int m, int k,
                   double radius, void* workspace, size_t workspace_bytes, uint8_t* spfh, void* stream) {
    if (!points || !normals || !idx || !workspace) return DICP_ERR_NULL;
    int rc = fpfh_check(dtype, idx64, c, N, m, k, radius);
    if (rc) return rc;
    if (workspace_bytes < fpfh_table_bytes(N, m)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(points, ts) || misaligned(normals, ts) || misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4))
        return DICP_ERR_ALIGN;
    const int R = spfh_rows_per_block(k), bpc = fpfh_blocks1(m, k);
    const unsigned g = (unsigned)N * (unsigned)bpc;
    const double radius2 = fpfh_radius2(radius);
    begin_launch();
    with_scalar_index(dtype, idx64, [&](auto t, auto i) {
        using T = decltype(t);
        using I = decltype(i);
        fpfh_spfh_kernel<T, I><<<g, BLOCK, 0, (hipStream_t)stream>>>((const T*)points, c, (const T*)normals, (const I*)idx, rows, m, k, R, bpc, radius2,
                                                                     (uint32_t*)workspace, spfh);
    });
    return launch_status();
}

int dicp_fpfh_combine(int dtype, const void* points, int c, const void* idx, int idx64, const int32_t* rows, int N, int m, int k, double radius,
                      const void* workspace, size_t workspace_bytes, void* out, void* stream) {
    if (!points || !idx || !workspace || !out) return DICP_ERR_NULL;
    int rc = fpfh_check(dtype, idx64, c, N, m, k, radius);
    if (rc) return rc;
    if (workspace_bytes < fpfh_table_bytes(N, m)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(points, ts) || misaligned(out, ts) || misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4))
        return DICP_ERR_ALIGN;
    const int bpc = fpfh_blocks2(m);
    const unsigned g = (unsigned)N * (unsigned)bpc;
    const double radius2 = fpfh_radius2(radius);
    begin_launch();
    with_scalar_index(dtype, idx64, [&](auto t, auto i) {
        using T = decltype(t);
        using I = decltype(i);
        fpfh_combine_kernel<T, I><<<g, WAVE, 0, (hipStream_t)stream>>>((const T*)points, c, (const I*)idx, rows, m, k, bpc, radius2, (const uint4*)workspace,
                                                                       (T*)out);
    });
    return launch_status();
}
