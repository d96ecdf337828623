// Outlier removal for batches of clouds (dicp_amd/filter.py): a stable mask compaction with its gradient, and the per-cloud statistics
// of the statistical filter.  The rules are csrc/dicp_filter.h.
//
// Compaction (dicp_select_rows), three launches over TILES of SELECT_TILE rows that never straddle two clouds -- no spin-waits and no
// hand-off between the blocks of a launch:
//   count   per tile: the kept rows (r < rows[b] and mask), from wave ballots
//   scan    per cloud (one block): the exclusive scan of its tiles' counts, any number of tiles in passes of SELECT_SCAN_THREADS with a
//           carried total -> the tiles' first output rows, rows_out
//   move    per tile: a kept row's rank from mbcnt on its wave's ballot and the waves' counts through LDS -> pos and index; then the
//           block copies its kept rows word by word (16-, 8- or 4-byte words, whatever the row size and the pointers allow), the
//           output side fully coalesced; then it zero-fills the output rows of its OWN tile range that lie at or past rows_out[b]
//           (index -1).  Every output element is stored exactly once; there is no separate fill.
// Gradient (dicp_select_rows_backward): one gather through pos, every element stored once.
//
// Statistics (dicp_outlier_stats):
//   row mean   one lane per row over the (N, m, k + 1) search result -> md (+inf for an invalid row) and the valid flags
//   compact    the valid rows' md in row order: the three compaction kernels above on 8-byte rows
//   sum64      one launch per round of partials (one lane per chunk of FILTER_CHUNK values, added in order), until one value per cloud
//              is left: first for the sum of md, then -- the first round squaring the deviations from the mean -- for the variance
//   mask       one lane per row: the cloud's threshold from the two sums (lane 0 of the cloud writes the statistics), the decision
// No float atomics: every result is bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_filter.h"

namespace {

constexpr int SEL_IPT = SELECT_TILE / BLOCK;       // rows per thread and tile
constexpr int SEL_NW = BLOCK / WAVE;
constexpr int SEL_MAX_COLS = 1 << 16;
static_assert(SELECT_TILE % BLOCK == 0 && SELECT_SCAN_THREADS == BLOCK, "the tile is whole rounds of the block; the scan runs on one block");

inline int sel_tiles(int m) { return (m + SELECT_TILE - 1) / SELECT_TILE; }

struct SelLayout { size_t tcnt, toff, total; };
inline SelLayout sel_layout(int N, int m) {
    SelLayout L;
    const size_t tiles = (size_t)N * sel_tiles(m);
    size_t off = 0;
    L.tcnt = off; off = up256(off + tiles * 4);
    L.toff = off; off = up256(off + tiles * 4);
    L.total = off;
    return L;
}

// the statistics' workspace: the flags and compacted values, the compaction's own, the partials of two rounds, the sums
struct OutLayout { size_t valid, vals, sel, V, part[2], sum_md, sum_sq, total; };
inline OutLayout out_layout(int N, int m) {
    OutLayout L;
    const size_t rows = (size_t)N * m;
    size_t off = 0;
    L.valid = off;   off = up256(off + rows);
    L.vals = off;    off = up256(off + rows * 8);
    L.sel = off;     off = up256(off + sel_layout(N, m).total);
    L.V = off;       off = up256(off + (size_t)N * 4);
    L.part[0] = off; off = up256(off + (size_t)N * filter_level_len(m, 1) * 8);
    L.part[1] = off; off = up256(off + (size_t)N * filter_level_len(m, 2) * 8);
    L.sum_md = off;  off = up256(off + (size_t)N * 8);
    L.sum_sq = off;  off = up256(off + (size_t)N * 8);
    L.total = off;
    return L;
}

template <typename W> __device__ __forceinline__ W zero_word();
template <> __device__ __forceinline__ uint4 zero_word<uint4>() { return make_uint4(0u, 0u, 0u, 0u); }
template <> __device__ __forceinline__ uint2 zero_word<uint2>() { return make_uint2(0u, 0u); }
template <> __device__ __forceinline__ uint32_t zero_word<uint32_t>() { return 0u; }

// lanes below this one whose bit is set
__device__ __forceinline__ int lane_rank(unsigned long long bal) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
}

// ------------------------------------------------------------------ count
__global__ __launch_bounds__(BLOCK) void sel_count_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ rows, int m, int tpc,
                                                          int32_t* __restrict__ tcnt) {
    __shared__ int wsum[SEL_NW];
    const int b = blockIdx.x / tpc, t = blockIdx.x - b * tpc;
    const int mb = rows_of(rows, b, m);
    const uint8_t* M = mask + (size_t)b * m;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < SEL_IPT; ++k) {
        const int i = t * SELECT_TILE + k * BLOCK + threadIdx.x;
        cnt += __popcll(__ballot(i < mb && M[i] != 0));
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int q = 0; q < SEL_NW; ++q) s += wsum[q];
        tcnt[blockIdx.x] = s;
    }
}

// ------------------------------------------------------------------ scan: one block per cloud
// exclusive prefix of v over the block's threads in thread order, and the block's total.  lds: BLOCK / WAVE ints
__device__ __forceinline__ int sel_block_excl_scan(int v, int* lds, int& total) {
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    int x = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == WAVE - 1) lds[w] = x;
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < SEL_NW; ++q) {
        const int s = lds[q];
        pre += q < w ? s : 0;
        tot += s;
    }
    __syncthreads();                                        // (lds is reused by the next pass)
    total = tot;
    return pre + x - v;
}

__global__ __launch_bounds__(SELECT_SCAN_THREADS) void sel_scan_kernel(int tpc, const int32_t* __restrict__ tcnt, int32_t* __restrict__ toff,
                                                                       int32_t* __restrict__ rows_out) {
    __shared__ int wsum[SEL_NW];
    const int b = blockIdx.x;
    const size_t q0 = (size_t)b * tpc;
    int run = 0;
    for (int t0 = 0; t0 < tpc; t0 += SELECT_SCAN_THREADS) {         // (block-uniform trip count)
        const int t = t0 + threadIdx.x;
        int tot;
        const int pre = sel_block_excl_scan(t < tpc ? tcnt[q0 + t] : 0, wsum, tot);
        if (t < tpc) toff[q0 + t] = run + pre;
        run += tot;
    }
    if (threadIdx.x == 0) rows_out[b] = run;
}

// ------------------------------------------------------------------ move
// src / dst: the rows as wpr words of type W each.  index / pos may be NULL.
template <typename W>
__global__ __launch_bounds__(BLOCK) void sel_move_kernel(const W* __restrict__ src, int wpr, const uint8_t* __restrict__ mask, const int32_t* __restrict__ rows,
                                                         int m, int tpc, const int32_t* __restrict__ toff, const int32_t* __restrict__ rows_out,
                                                         W* __restrict__ dst, int64_t* __restrict__ index, int32_t* __restrict__ pos) {
    __shared__ int wcnt[SEL_IPT][SEL_NW];
    __shared__ int lsrc[SELECT_TILE];
    const int b = blockIdx.x / tpc, t = blockIdx.x - b * tpc;
    const int mb = rows_of(rows, b, m);
    const size_t base = (size_t)b * m;
    const int i0 = t * SELECT_TILE;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    bool keep[SEL_IPT];
    int rank[SEL_IPT];
#pragma unroll
    for (int k = 0; k < SEL_IPT; ++k) {
        const int i = i0 + k * BLOCK + threadIdx.x;
        keep[k] = i < mb && mask[base + i] != 0;
        const unsigned long long bal = __ballot(keep[k]);
        rank[k] = lane_rank(bal);
        if (lane == 0) wcnt[k][w] = __popcll(bal);
    }
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int k = 0; k < SEL_IPT; ++k) {
#pragma unroll
        for (int q = 0; q < SEL_NW; ++q) {
            if (q == w) rank[k] += tot;                     // (rows before this wave's round, in row order)
            tot += wcnt[k][q];
        }
    }
    const int run = toff[blockIdx.x];                       // (run + tot <= rows_out[b] <= m)
#pragma unroll
    for (int k = 0; k < SEL_IPT; ++k) {
        const int i = i0 + k * BLOCK + threadIdx.x;
        if (i >= m) continue;
        if (keep[k]) {
            lsrc[rank[k]] = i;
            if (index) index[base + run + rank[k]] = i;
        }
        if (pos) pos[base + i] = keep[k] ? run + rank[k] : -1;
    }
    __syncthreads();
    // the kept rows, word by word: thread e takes word e % wpr of kept row e / wpr, then 256 words on
    const int dr = BLOCK / wpr, dw = BLOCK - dr * wpr;
    {
        const W* S = src + base * wpr;
        W* D = dst + (base + run) * wpr;
        const int nw = tot * wpr;
        int r = threadIdx.x / wpr, c = threadIdx.x - r * wpr;
        for (int e = threadIdx.x; e < nw; e += BLOCK) {
            D[e] = S[(size_t)lsrc[r] * wpr + c];
            r += dr; c += dw;
            if (c >= wpr) { c -= wpr; ++r; }
        }
    }
    // the output rows of this tile's own range at or past the cloud's count
    const int z0 = max(i0, min(max(rows_out[b], 0), m)), z1 = min(i0 + SELECT_TILE, m);
    if (z0 < z1) {
        W* Z = dst + (base + z0) * wpr;
        const int nw = (z1 - z0) * wpr;
        const W zero = zero_word<W>();
        for (int e = threadIdx.x; e < nw; e += BLOCK) Z[e] = zero;
        if (index)
            for (int j = z0 + threadIdx.x; j < z1; j += BLOCK) index[base + j] = -1;
    }
}

// ------------------------------------------------------------------ backward: grad[b, i] = g[b, pos[b, i]], 0 for a row that was dropped
template <typename W>
__global__ __launch_bounds__(BLOCK) void sel_backward_kernel(const W* __restrict__ g, int wpr, const int32_t* __restrict__ pos, int m, int tpc,
                                                             W* __restrict__ grad) {
    __shared__ int lp[SELECT_TILE];
    const int b = blockIdx.x / tpc, t = blockIdx.x - b * tpc;
    const size_t base = (size_t)b * m;
    const int i0 = t * SELECT_TILE;
    const int nrows = min(SELECT_TILE, m - i0);
    for (int j = threadIdx.x; j < nrows; j += BLOCK) {
        const int p = pos[base + i0 + j];
        lp[j] = p < m ? p : -1;                             // (in range whatever pos holds)
    }
    __syncthreads();
    const W* G = g + base * wpr;
    W* D = grad + (base + i0) * wpr;
    const int nw = nrows * wpr;
    const int dr = BLOCK / wpr, dw = BLOCK - dr * wpr;
    const W zero = zero_word<W>();
    int r = threadIdx.x / wpr, c = threadIdx.x - r * wpr;
    for (int e = threadIdx.x; e < nw; e += BLOCK) {
        const int p = lp[r];
        W v = zero;
        if (p >= 0) v = G[(size_t)p * wpr + c];
        D[e] = v;
        r += dr; c += dw;
        if (c >= wpr) { c -= wpr; ++r; }
    }
}

// the widest word both the row size and every pointer allow: 16, 8 or 4 bytes
inline int sel_word_bytes(size_t row_bytes, const void* a, const void* b) {
    const uintptr_t x = (uintptr_t)a | (uintptr_t)b | (uintptr_t)row_bytes;
    return !(x & 15) ? 16 : (!(x & 7) ? 8 : 4);
}
template <typename F>
inline void with_word(int bytes, F&& f) {
    if (bytes == 16) f(uint4());
    else if (bytes == 8) f(uint2());
    else f(uint32_t());
}

int sel_check(int N, int m) {
    if (N <= 0 || m <= 0 || m >= 0x7fffffff - SELECT_TILE) return DICP_ERR_SHAPE;
    if ((size_t)N * (size_t)sel_tiles(m) > (size_t)0x7fffffff) return DICP_ERR_SHAPE;      // one block per tile
    return 0;
}

// count, scan and move on checked arguments
void sel_launch(const void* src, size_t row_bytes, const uint8_t* mask, const int32_t* rows, int N, int m, void* dst, int32_t* rows_out,
                int64_t* index, int32_t* pos, char* ws, hipStream_t st) {
    const SelLayout L = sel_layout(N, m);
    const int tpc = sel_tiles(m);
    const unsigned g = (unsigned)N * (unsigned)tpc;
    int32_t* tcnt = (int32_t*)(ws + L.tcnt);
    int32_t* toff = (int32_t*)(ws + L.toff);
    sel_count_kernel<<<g, BLOCK, 0, st>>>(mask, rows, m, tpc, tcnt);
    sel_scan_kernel<<<N, SELECT_SCAN_THREADS, 0, st>>>(tpc, tcnt, toff, rows_out);
    const int wb = sel_word_bytes(row_bytes, src, dst);
    with_word(wb, [&](auto wd) {
        using W = decltype(wd);
        sel_move_kernel<W><<<g, BLOCK, 0, st>>>((const W*)src, (int)(row_bytes / wb), mask, rows, m, tpc, toff, rows_out, (W*)dst, index, pos);
    });
}

// ------------------------------------------------------------------ statistics
inline int out_blocks(int m) { return (m + BLOCK - 1) / BLOCK; }

template <typename T>
__global__ __launch_bounds__(BLOCK) void out_row_mean_kernel(const T* __restrict__ d2, const int64_t* __restrict__ idx, const int32_t* __restrict__ rows,
                                                             int m, int bpc, int k, double* __restrict__ md, uint8_t* __restrict__ valid) {
    const int b = blockIdx.x / bpc, i = (blockIdx.x - b * bpc) * BLOCK + threadIdx.x;
    if (i >= m) return;
    const size_t r = (size_t)b * m + i;
    int cnt = 0;
    double v = (double)INFINITY;
    if (i < rows_of(rows, b, m)) v = outlier_row_mean<T>(d2 + r * (k + 1), idx + r * (k + 1), (int64_t)i, k, &cnt);
    md[r] = v;
    valid[r] = cnt > 0 ? 1 : 0;
}

// round `level` >= 1 of sum64: partial j of cloud b over its list of round level - 1 (round 0: the V compacted values; SQ: their squared
// deviations from the mean).  cap: the partials a cloud of m valid rows would have.  Partial 0 is always written (an empty list: +0).
template <bool SQ>
__global__ __launch_bounds__(BLOCK) void out_level_kernel(const double* __restrict__ in, size_t in_stride, const int32_t* __restrict__ V, int level,
                                                          int cap, int bpc, const double* __restrict__ sum_md, double* __restrict__ out, size_t out_stride) {
    const int b = blockIdx.x / bpc, j = (blockIdx.x - b * bpc) * BLOCK + threadIdx.x;
    if (j >= cap) return;
    const int64_t len = filter_level_len((int64_t)V[b], level - 1);
    const int64_t rest = len - (int64_t)j * FILTER_CHUNK;
    if (j > 0 && rest <= 0) return;
    const int n = (int)(rest < 0 ? 0 : (rest < FILTER_CHUNK ? rest : FILTER_CHUNK));
    const double* v = in + (size_t)b * in_stride + (size_t)j * FILTER_CHUNK;
    out[(size_t)b * out_stride + j] = SQ ? filter_chunk_sqdev(v, n, outlier_mean(sum_md[b], (int64_t)V[b])) : filter_chunk_sum(v, n);
}

__global__ __launch_bounds__(BLOCK) void out_mask_kernel(const double* __restrict__ md, const uint8_t* __restrict__ valid, const int32_t* __restrict__ V,
                                                         const double* __restrict__ sum_md, const double* __restrict__ sum_sq, double std_ratio,
                                                         int m, int bpc, double* __restrict__ stats, uint8_t* __restrict__ mask) {
    const int b = blockIdx.x / bpc, i = (blockIdx.x - b * bpc) * BLOCK + threadIdx.x;
    if (i >= m) return;
    const int64_t v = (int64_t)V[b];
    double s[OUTLIER_STATS];
    outlier_stats(outlier_mean(sum_md[b], v), sum_sq[b], v, std_ratio, s);
    if (i == 0) {
#pragma unroll
        for (int q = 0; q < OUTLIER_STATS; ++q) stats[(size_t)b * OUTLIER_STATS + q] = s[q];
    }
    const size_t r = (size_t)b * m + i;
    mask[r] = outlier_keep(valid[r] != 0, md[r], s[2]) ? 1 : 0;
}

int out_check(int dtype, int N, int m, int k) {
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    int rc = sel_check(N, m);
    if (rc) return rc;
    if (k < OUTLIER_K_MIN || k > OUTLIER_K_MAX) return DICP_ERR_SHAPE;
    if ((size_t)N * (size_t)out_blocks(m) > (size_t)0x7fffffff) return DICP_ERR_SHAPE;     // one lane per row
    return 0;
}

// the rounds of sum64 over the compacted values: -> sum (N)
template <bool SQ>
void out_sum64(const double* vals, const int32_t* V, int N, int m, const double* sum_md, double* part0, double* part1, double* sum, hipStream_t st) {
    const int levels = filter_levels(m);
    double* part[2] = {part0, part1};
    const double* in = vals;
    size_t in_stride = (size_t)m;
    for (int l = 1; l <= levels; ++l) {
        const int cap = (int)filter_level_len(m, l);
        double* out = l == levels ? sum : part[(l - 1) & 1];
        const int bpc = out_blocks(cap);
        const unsigned g = (unsigned)N * (unsigned)bpc;
        if (SQ && l == 1) out_level_kernel<true><<<g, BLOCK, 0, st>>>(in, in_stride, V, l, cap, bpc, sum_md, out, (size_t)cap);
        else              out_level_kernel<false><<<g, BLOCK, 0, st>>>(in, in_stride, V, l, cap, bpc, sum_md, out, (size_t)cap);
        in = out;
        in_stride = (size_t)cap;
    }
}

}  // namespace

size_t dicp_select_workspace_bytes(int N, int m) {
    if (sel_check(N, m)) return 0;
    return sel_layout(N, m).total;
}

int dicp_select_rows(int dtype, const void* pts, int c, const uint8_t* mask, const int32_t* rows, int N, int m, void* out, int32_t* rows_out,
                     int64_t* index, int32_t* pos, void* workspace, size_t workspace_bytes, void* stream) {
    if (!pts || !mask || !out || !rows_out || !workspace) return DICP_ERR_NULL;
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    int rc = sel_check(N, m);
    if (rc) return rc;
    if (c < 1 || c > SEL_MAX_COLS || pts == out) return DICP_ERR_SHAPE;
    if (workspace_bytes < sel_layout(N, m).total) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(pts, ts) || misaligned(out, ts) || misaligned(rows, 4) || misaligned(rows_out, 4)
        || misaligned(index, 8) || misaligned(pos, 4)) return DICP_ERR_ALIGN;
    begin_launch();
    sel_launch(pts, (size_t)c * ts, mask, rows, N, m, out, rows_out, index, pos, (char*)workspace, (hipStream_t)stream);
    return launch_status();
}

int dicp_select_rows_backward(int dtype, const void* grad_out, const int32_t* pos, int N, int m, int c, void* grad_pts, void* stream) {
    if (!grad_out || !pos || !grad_pts) return DICP_ERR_NULL;
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    int rc = sel_check(N, m);
    if (rc) return rc;
    if (c < 1 || c > SEL_MAX_COLS || grad_out == grad_pts) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(grad_out, ts) || misaligned(grad_pts, ts) || misaligned(pos, 4)) return DICP_ERR_ALIGN;
    const int tpc = sel_tiles(m);
    const unsigned g = (unsigned)N * (unsigned)tpc;
    const size_t row_bytes = (size_t)c * ts;
    const int wb = sel_word_bytes(row_bytes, grad_out, grad_pts);
    begin_launch();
    with_word(wb, [&](auto wd) {
        using W = decltype(wd);
        sel_backward_kernel<W><<<g, BLOCK, 0, (hipStream_t)stream>>>((const W*)grad_out, (int)(row_bytes / wb), pos, m, tpc, (W*)grad_pts);
    });
    return launch_status();
}

size_t dicp_outlier_workspace_bytes(int N, int m) {
    if (sel_check(N, m) || (size_t)N * (size_t)out_blocks(m) > (size_t)0x7fffffff) return 0;
    return out_layout(N, m).total;
}

int dicp_outlier_stats(int dtype, const void* d2, const int64_t* idx, const int32_t* rows, int N, int m, int k, double std_ratio,
                       double* mean_distance, double* stats, uint8_t* mask, void* workspace, size_t workspace_bytes, void* stream) {
    if (!d2 || !idx || !mean_distance || !stats || !mask || !workspace) return DICP_ERR_NULL;
    int rc = out_check(dtype, N, m, k);
    if (rc) return rc;
    if (!(std_ratio >= 0.0 && std_ratio < HUGE_VAL)) return DICP_ERR_SHAPE;
    const OutLayout L = out_layout(N, m);
    if (workspace_bytes < L.total) return DICP_ERR_SHAPE;
    if (misaligned(workspace, 256) || misaligned(d2, elem_size(dtype)) || misaligned(idx, 8) || misaligned(rows, 4) || misaligned(mean_distance, 8)
        || misaligned(stats, 8)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint8_t* valid = (uint8_t*)(ws + L.valid);
    double* vals = (double*)(ws + L.vals);
    int32_t* V = (int32_t*)(ws + L.V);
    double* part0 = (double*)(ws + L.part[0]);
    double* part1 = (double*)(ws + L.part[1]);
    double* sum_md = (double*)(ws + L.sum_md);
    double* sum_sq = (double*)(ws + L.sum_sq);
    const int bpc = out_blocks(m);
    const unsigned g = (unsigned)N * (unsigned)bpc;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        out_row_mean_kernel<T><<<g, BLOCK, 0, st>>>((const T*)d2, idx, rows, m, bpc, k, mean_distance, valid);
    });
    sel_launch(mean_distance, 8, valid, rows, N, m, vals, V, nullptr, nullptr, ws + L.sel, st);
    out_sum64<false>(vals, V, N, m, nullptr, part0, part1, sum_md, st);
    out_sum64<true>(vals, V, N, m, sum_md, part0, part1, sum_sq, st);
    out_mask_kernel<<<g, BLOCK, 0, st>>>(mean_distance, valid, V, sum_md, sum_sq, std_ratio, m, bpc, stats, mask);
    return launch_status();
}
