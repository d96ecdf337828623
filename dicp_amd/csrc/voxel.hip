// Voxel-grid downsampling of batches of clouds (dicp_amd/voxel.py): every cloud's rows binned by floor((p - o) / s), one centroid
// (the mean of all c columns) per occupied voxel, in ascending (vx, vy, vz) order -- and the gradient back to the rows.
//
// Count phase (dicp_voxel_count), every kernel over TILES of VOX_TILE rows that never straddle two clouds, so that a single
// large cloud spreads over many blocks like a batch of small ones:
//   bounds    per tile: min / max of the voxel coordinates of its valid rows (r < rows[b], finite x, y, z), their count, range errors
//   plan      per cloud (one block): the tiles' reduction -> widths, key bits, radix passes, error code; each tile's base among the
//             cloud's valid rows
//   keys      per tile: the valid rows' 64-bit keys (csrc/dicp_voxel.h), compacted stably to the cloud's first nv slots with their row
//             index (invalid rows never enter the sort)
//   sort      per 8-bit digit of the key, only the passes the cloud needs (others exit at once): per-tile digit histograms, a per-cloud
//             scan of (digit, tile) -> the tile's first slot per digit, a stable scatter (each 256-row round ranked by wave ballots)
//   segments  per tile: head flags (a key unlike its predecessor) -> per-cloud scan -> each voxel's first sorted slot; with
//             min_points > 1 the same tile/scan pattern over the voxels keeps those with enough rows
//   finish    rows_out (N) and the error word: what the host reads, once, to size the outputs
// Reduce phase (dicp_voxel_reduce), into the caller's (N, M, c) / (N, M) / (N, m) outputs:
//   small     one lane per output voxel of <= VOX_SMALL rows: the sum of its rows' columns in double in sorted (= row) order,
//             / count, rounded once; its rows' inverse entries.  Larger voxels go on a list (an integer counter)
//   big       one block per listed voxel: lane t sums rows t, t + 256, ... in order, then a fixed LDS tree -- the same order whichever
//             block takes the voxel, so the result does not depend on scheduling
// Backward (dicp_voxel_backward): one lane per input row, grad = g[inverse] / count.  No float atomics anywhere: forward and
// backward are bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_fill.h"
#include "dicp_voxel.h"

namespace {

constexpr int VOX_IPT = 16;                        // rows per thread and tile
constexpr int VOX_TILE = BLOCK * VOX_IPT;          // 4096 rows
constexpr int VOX_SMALL = 64;                      // voxels of up to this many rows: one lane each
constexpr int VOX_MAX_PASSES = 8;
constexpr int VOX_SCAN_THREADS = 1024;             // the digit scan: 4 groups of tiles x 256 digits
constexpr int VOX_BIG_BLOCKS = 1024;

// per-cloud record, VOX_CI int32 words
enum { CI_NV = 0, CI_PASSES = 1, CI_WY = 2, CI_WZ = 3, CI_V = 4, CI_OUT = 5, CI_ERR = 6, VOX_CI = 8 };
enum { VOX_ERR_RANGE = 1, VOX_ERR_BITS = 2 };

inline int vox_tiles(int m) { return (m + VOX_TILE - 1) / VOX_TILE; }
inline size_t vox_big_cap(int N, int m) { return (size_t)N * m / (VOX_SMALL + 1) + 1; }

// block -> (cloud, tile): consecutive blocks take one cloud's tiles (not decode_block's XCD grouping, which would put all of a single
// large cloud on one XCD)
__device__ __forceinline__ bool vox_decode(int tpc, int N, int& b, int& t) {
    b = blockIdx.x / tpc;
    t = blockIdx.x - b * tpc;
    return b < N;
}
inline unsigned vox_grid(int N, int tpc) { return (unsigned)N * (unsigned)tpc; }

// The workspace, each part 256-byte aligned; the reduce phase reads what the count phase left in it
struct VoxLayout {
    size_t key[2], idx[2], start, vidof, tmin, tmax, tcnt, tbad, toff, hist, cinfo, vlo, big, bigcount, total;
};
inline VoxLayout vox_layout(int N, int m) {
    VoxLayout L;
    const size_t rows = (size_t)N * m, tiles = (size_t)N * vox_tiles(m);
    size_t off = 0;
    for (int p = 0; p < 2; ++p) { L.key[p] = off; off = up256(off + rows * 8); }
    for (int p = 0; p < 2; ++p) { L.idx[p] = off; off = up256(off + rows * 4); }
    L.start = off;    off = up256(off + (size_t)N * (m + 1) * 4);
    L.vidof = off;    off = up256(off + rows * 4);
    L.tmin = off;     off = up256(off + tiles * 3 * 8);
    L.tmax = off;     off = up256(off + tiles * 3 * 8);
    L.tcnt = off;     off = up256(off + tiles * 4);
    L.tbad = off;     off = up256(off + tiles * 4);
    L.toff = off;     off = up256(off + tiles * 4);
    L.hist = off;     off = up256(off + tiles * 256 * 4);
    L.cinfo = off;    off = up256(off + (size_t)N * VOX_CI * 4);
    L.vlo = off;      off = up256(off + (size_t)N * 3 * 8);
    L.big = off;      off = up256(off + vox_big_cap(N, m) * 2 * 4);
    L.bigcount = off; off = up256(off + 4);
    L.total = off;
    return L;
}

// ------------------------------------------------------------------ block helpers (blockDim = NT, a multiple of 64)
// exclusive prefix of v over the block's threads in thread order, and the block's total.  lds: NT / 64 ints
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int* lds, int& total) {
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
    for (int k = 0; k < NT / WAVE; ++k) {
        const int s = lds[k];
        pre += k < w ? s : 0;
        tot += s;
    }
    __syncthreads();                                        // (lds is reused by the next call)
    total = tot;
    return pre + x - v;
}

// the same for a 0/1 flag, by ballots
__device__ __forceinline__ int block_flag_prefix(bool f, int* lds, int& total) {
    const unsigned long long bal = __ballot(f);
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    if (lane == 0) lds[w] = __popcll(bal);
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < BLOCK / WAVE; ++k) {
        const int s = lds[k];
        pre += k < w ? s : 0;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return pre + __popcll(bal & ((1ull << lane) - 1ull));
}

template <typename T>
__device__ __forceinline__ bool vox_finite(T x) { return x - x == T(0); }       // false for inf and NaN

// the row's validity and voxel coordinates (ok: every coordinate in range)
template <typename T>
__device__ __forceinline__ bool vox_row(const T* __restrict__ p, const T* so, int64_t* v, bool& ok) {
    const T x = p[0], y = p[1], z = p[2];
    if (!(vox_finite(x) && vox_finite(y) && vox_finite(z))) { ok = true; return false; }
    ok = vox_coord<T>(x, so[3], so[0], v) & vox_coord<T>(y, so[4], so[1], v + 1) & vox_coord<T>(z, so[5], so[2], v + 2);
    return true;
}

// so = [s_x, s_y, s_z, o_x, o_y, o_z] of cloud b in T
template <typename T>
__device__ __forceinline__ void vox_so(T sx, T sy, T sz, const T* __restrict__ origin, int o_stride, int b, T* so) {
    so[0] = sx; so[1] = sy; so[2] = sz;
    const T* o = origin ? origin + (size_t)b * o_stride : nullptr;
    so[3] = o ? o[0] : T(0); so[4] = o ? o[1] : T(0); so[5] = o ? o[2] : T(0);
}

// ------------------------------------------------------------------ bounds
template <typename T>
__global__ __launch_bounds__(BLOCK) void vox_bounds_kernel(const T* __restrict__ pts, int c, const int32_t* __restrict__ rows, int N, int m, int tpc,
                                                           T sx, T sy, T sz, const T* __restrict__ origin, int o_stride,
                                                           int64_t* __restrict__ tmin, int64_t* __restrict__ tmax, int32_t* __restrict__ tcnt,
                                                           int32_t* __restrict__ tbad) {
    __shared__ long long lmin[3][BLOCK / WAVE], lmax[3][BLOCK / WAVE];
    __shared__ int lcnt[BLOCK / WAVE], lbad[BLOCK / WAVE];
    int b, t;
    if (!vox_decode(tpc, N, b, t)) return;
    const int mb = rows_of(rows, b, m);
    T so[6];
    vox_so(sx, sy, sz, origin, o_stride, b, so);
    long long lo[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, hi[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
    int cnt = 0, bad = 0;
    for (int k = 0; k < VOX_IPT; ++k) {
        const int i = t * VOX_TILE + k * BLOCK + threadIdx.x;
        if (i >= mb) break;
        int64_t v[3];
        bool ok;
        if (!vox_row<T>(pts + ((size_t)b * m + i) * c, so, v, ok)) continue;
        ++cnt;
        if (!ok) { bad = 1; continue; }
#pragma unroll
        for (int d = 0; d < 3; ++d) { lo[d] = min(lo[d], (long long)v[d]); hi[d] = max(hi[d], (long long)v[d]); }
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { lo[d] = min(lo[d], __shfl_xor(lo[d], off)); hi[d] = max(hi[d], __shfl_xor(hi[d], off)); }
        cnt += __shfl_xor(cnt, off);
        bad |= __shfl_xor(bad, off);
    }
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    if (lane == 0) {
        for (int d = 0; d < 3; ++d) { lmin[d][w] = lo[d]; lmax[d][w] = hi[d]; }
        lcnt[w] = cnt; lbad[w] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t q = (size_t)b * tpc + t;
        int cs = 0, bs = 0;
        for (int d = 0; d < 3; ++d) {
            long long a = INT64_MAX, z = INT64_MIN;
            for (int k = 0; k < BLOCK / WAVE; ++k) { a = min(a, lmin[d][k]); z = max(z, lmax[d][k]); }
            tmin[q * 3 + d] = a; tmax[q * 3 + d] = z;
        }
        for (int k = 0; k < BLOCK / WAVE; ++k) { cs += lcnt[k]; bs |= lbad[k]; }
        tcnt[q] = cs; tbad[q] = bs;
    }
}

// ------------------------------------------------------------------ plan: one block per cloud
__global__ __launch_bounds__(BLOCK) void vox_plan_kernel(int N, int tpc, const int64_t* __restrict__ tmin, const int64_t* __restrict__ tmax,
                                                         const int32_t* __restrict__ tcnt, const int32_t* __restrict__ tbad,
                                                         int32_t* __restrict__ toff, int32_t* __restrict__ cinfo, int64_t* __restrict__ vlo) {
    __shared__ long long lmin[3][BLOCK], lmax[3][BLOCK];
    __shared__ int lbad[BLOCK];
    __shared__ int wsum[BLOCK / WAVE];
    const int b = blockIdx.x;
    const size_t q0 = (size_t)b * tpc;
    long long lo[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, hi[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
    int bad = 0, run = 0;
    for (int t0 = 0; t0 < tpc; t0 += BLOCK) {               // (block-uniform trip count)
        const int t = t0 + threadIdx.x;
        const int n = t < tpc ? tcnt[q0 + t] : 0;
        if (t < tpc) {
#pragma unroll
            for (int d = 0; d < 3; ++d) { lo[d] = min(lo[d], (long long)tmin[(q0 + t) * 3 + d]); hi[d] = max(hi[d], (long long)tmax[(q0 + t) * 3 + d]); }
            bad |= tbad[q0 + t];
        }
        int tot;
        const int pre = block_excl_scan<BLOCK>(n, wsum, tot);
        if (t < tpc) toff[q0 + t] = run + pre;
        run += tot;
    }
    for (int d = 0; d < 3; ++d) { lmin[d][threadIdx.x] = lo[d]; lmax[d][threadIdx.x] = hi[d]; }
    lbad[threadIdx.x] = bad;
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            for (int d = 0; d < 3; ++d) {
                lmin[d][threadIdx.x] = min(lmin[d][threadIdx.x], lmin[d][threadIdx.x + s]);
                lmax[d][threadIdx.x] = max(lmax[d][threadIdx.x], lmax[d][threadIdx.x + s]);
            }
            lbad[threadIdx.x] |= lbad[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int32_t* ci = cinfo + (size_t)b * VOX_CI;
        int err = lbad[0] ? VOX_ERR_RANGE : 0;
        int w[3] = {0, 0, 0};
        int64_t l[3] = {0, 0, 0};
        if (run > 0 && !err) {
            for (int d = 0; d < 3; ++d) { l[d] = lmin[d][0]; w[d] = vox_width(lmin[d][0], lmax[d][0]); }
            if (!vox_widths_ok(w[0], w[1], w[2])) err = VOX_ERR_BITS;
        }
        if (err) { w[0] = w[1] = w[2] = 0; l[0] = l[1] = l[2] = 0; }
        ci[CI_NV] = run;
        ci[CI_PASSES] = vox_passes(w[0], w[1], w[2]);
        ci[CI_WY] = w[1]; ci[CI_WZ] = w[2];
        ci[CI_V] = 0; ci[CI_OUT] = 0; ci[CI_ERR] = err;
        for (int d = 0; d < 3; ++d) vlo[(size_t)b * 3 + d] = l[d];
    }
}

// ------------------------------------------------------------------ keys: the valid rows, compacted stably
template <typename T>
__global__ __launch_bounds__(BLOCK) void vox_keys_kernel(const T* __restrict__ pts, int c, const int32_t* __restrict__ rows, int N, int m, int tpc,
                                                         T sx, T sy, T sz, const T* __restrict__ origin, int o_stride,
                                                         const int32_t* __restrict__ toff, const int32_t* __restrict__ cinfo, const int64_t* __restrict__ vlo,
                                                         uint64_t* __restrict__ key, int32_t* __restrict__ idx) {
    __shared__ int wsum[BLOCK / WAVE];
    int b, t;
    if (!vox_decode(tpc, N, b, t)) return;
    const int mb = rows_of(rows, b, m);
    if (t * VOX_TILE >= mb) return;                         // (block-uniform)
    T so[6];
    vox_so(sx, sy, sz, origin, o_stride, b, so);
    const int32_t* ci = cinfo + (size_t)b * VOX_CI;
    const int wy = ci[CI_WY], wz = ci[CI_WZ];
    const int64_t lo[3] = {vlo[(size_t)b * 3], vlo[(size_t)b * 3 + 1], vlo[(size_t)b * 3 + 2]};
    int run = toff[(size_t)b * tpc + t];
    const size_t base = (size_t)b * m;
    for (int k = 0; k < VOX_IPT; ++k) {
        const int i = t * VOX_TILE + k * BLOCK + threadIdx.x;
        int64_t v[3] = {0, 0, 0};
        bool ok = true;
        const bool valid = i < mb && vox_row<T>(pts + (base + i) * c, so, v, ok);
        int tot;
        const int pos = run + block_flag_prefix(valid, wsum, tot);
        if (valid) {
            key[base + pos] = ok ? vox_key(v, lo, wy, wz) : 0;     // (a cloud with a range error is reported, never reduced)
            idx[base + pos] = i;
        }
        run += tot;
    }
}

// ------------------------------------------------------------------ sort: one 8-bit digit per pass
__global__ __launch_bounds__(BLOCK) void vox_hist_kernel(int N, int m, int tpc, int pass, const int32_t* __restrict__ cinfo,
                                                         const uint64_t* __restrict__ key, int32_t* __restrict__ hist) {
    __shared__ int h[256];
    int b, t;
    if (!vox_decode(tpc, N, b, t)) return;
    const int32_t* ci = cinfo + (size_t)b * VOX_CI;
    if (pass >= ci[CI_PASSES]) return;                      // (block-uniform)
    const int nv = ci[CI_NV], shift = 8 * pass;
    h[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)b * m;
    for (int k = 0; k < VOX_IPT; ++k) {
        const int i = t * VOX_TILE + k * BLOCK + threadIdx.x;
        if (i < nv) atomicAdd(&h[(int)((key[base + i] >> shift) & 255u)], 1);
    }
    __syncthreads();
    hist[((size_t)b * tpc + t) * 256 + threadIdx.x] = h[threadIdx.x];
}

// hist (N, tpc, 256) counts -> each tile's first slot per digit within its cloud (in place): digit-major, tile-minor
__global__ __launch_bounds__(VOX_SCAN_THREADS) void vox_digit_scan_kernel(int tpc, int pass, const int32_t* __restrict__ cinfo, int32_t* __restrict__ hist) {
    constexpr int G = VOX_SCAN_THREADS / 256;
    __shared__ int part[G][256];
    __shared__ int wsum[VOX_SCAN_THREADS / WAVE];
    const int b = blockIdx.x;
    if (pass >= cinfo[(size_t)b * VOX_CI + CI_PASSES]) return;      // (block-uniform)
    const int g = threadIdx.x / 256, d = threadIdx.x % 256;
    const int chunk = (tpc + G - 1) / G, t0 = min(g * chunk, tpc), t1 = min(t0 + chunk, tpc);
    int32_t* H = hist + (size_t)b * tpc * 256;
    int s = 0;
    for (int t = t0; t < t1; ++t) s += H[(size_t)t * 256 + d];
    part[g][d] = s;
    __syncthreads();
    int total = 0, pre = 0;
#pragma unroll
    for (int k = 0; k < G; ++k) { const int x = part[k][d]; pre += k < g ? x : 0; total += x; }
    int all;
    const int dbase = block_excl_scan<VOX_SCAN_THREADS>(g == 0 ? total : 0, wsum, all);     // (threads of g = 0 first: digit order)
    __shared__ int bases[256];
    if (g == 0) bases[d] = dbase;
    __syncthreads();
    int run = bases[d] + pre;
    for (int t = t0; t < t1; ++t) {
        const int x = H[(size_t)t * 256 + d];
        H[(size_t)t * 256 + d] = run;
        run += x;
    }
}

// stable scatter of the pass's digit: rounds of 256 rows in order, each ranked within its wave by 8 ballots and across the waves
// through LDS counts
__global__ __launch_bounds__(BLOCK) void vox_scatter_kernel(int N, int m, int tpc, int pass, const int32_t* __restrict__ cinfo, const int32_t* __restrict__ hist,
                                                            const uint64_t* __restrict__ key_in, const int32_t* __restrict__ idx_in,
                                                            uint64_t* __restrict__ key_out, int32_t* __restrict__ idx_out) {
    constexpr int NW = BLOCK / WAVE;
    __shared__ int dbase[256];
    __shared__ int wcnt[NW][256];
    int b, t;
    if (!vox_decode(tpc, N, b, t)) return;
    const int32_t* ci = cinfo + (size_t)b * VOX_CI;
    if (pass >= ci[CI_PASSES]) return;                      // (block-uniform)
    const int nv = ci[CI_NV], shift = 8 * pass;
    if (t * VOX_TILE >= nv) return;                         // (block-uniform)
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    dbase[threadIdx.x] = hist[((size_t)b * tpc + t) * 256 + threadIdx.x];
#pragma unroll
    for (int k = 0; k < NW; ++k) wcnt[k][threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)b * m;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int k = 0; k < VOX_IPT; ++k) {
        const int i = t * VOX_TILE + k * BLOCK + threadIdx.x;
        const bool act = i < nv;
        uint64_t kk = 0;
        int id = 0;
        if (act) { kk = key_in[base + i]; id = idx_in[base + i]; }
        const int dg = act ? (int)((kk >> shift) & 255u) : 0;
        unsigned long long peers = __ballot(act);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (dg >> bit) & 1;
            const unsigned long long bal = __ballot(on);
            peers &= on ? bal : ~bal;
        }
        const int rank = __popcll(peers & lt);
        if (act && rank == 0) wcnt[w][dg] = __popcll(peers);
        __syncthreads();
        if (act) {
            int pos = dbase[dg] + rank;
            for (int q = 0; q < w; ++q) pos += wcnt[q][dg];
            key_out[base + pos] = kk;
            idx_out[base + pos] = id;
        }
        __syncthreads();
        int s = 0;
#pragma unroll
        for (int q = 0; q < NW; ++q) { s += wcnt[q][threadIdx.x]; wcnt[q][threadIdx.x] = 0; }
        dbase[threadIdx.x] += s;
        __syncthreads();
    }
}

// ------------------------------------------------------------------ segments
// MODE_HEAD: items = the cloud's nv sorted slots, flag = a key unlike its predecessor; writes start[voxel] = slot (and vidof = identity
//            when nothing is filtered), start[V] = nv.
// MODE_KEEP: items = the cloud's V voxels, flag = at least min_points rows; writes vidof[output] = voxel.
enum { MODE_HEAD = 0, MODE_KEEP = 1 };

template <int MODE>
__device__ __forceinline__ bool vox_flag(int i, const uint64_t* __restrict__ key, const int32_t* __restrict__ start, int min_points) {
    if (MODE == MODE_HEAD) return i == 0 || key[i] != key[i - 1];
    return start[i + 1] - start[i] >= min_points;
}

template <int MODE>
__global__ __launch_bounds__(BLOCK) void vox_seg_count_kernel(int N, int m, int tpc, const int32_t* __restrict__ cinfo, const uint64_t* __restrict__ key0,
                                                              const uint64_t* __restrict__ key1, const int32_t* __restrict__ start, int min_points,
                                                              int32_t* __restrict__ tcnt) {
    __shared__ int wsum[BLOCK / WAVE];
    int b, t;
    if (!vox_decode(tpc, N, b, t)) return;
    const int32_t* ci = cinfo + (size_t)b * VOX_CI;
    const int n = MODE == MODE_HEAD ? ci[CI_NV] : ci[CI_V];
    const uint64_t* key = ((ci[CI_PASSES] & 1) ? key1 : key0) + (size_t)b * m;
    const int32_t* st = start + (size_t)b * (m + 1);
    int cnt = 0;
    for (int k = 0; k < VOX_IPT; ++k) {
        const int i = t * VOX_TILE + k * BLOCK + threadIdx.x;
        if (i < n && vox_flag<MODE>(i, key, st, min_points)) ++cnt;
    }
    int tot;
    block_excl_scan<BLOCK>(cnt, wsum, tot);
    if (threadIdx.x == 0) tcnt[(size_t)b * tpc + t] = tot;
}

// per cloud: exclusive scan of the tiles' counts -> toff, the total -> cinfo[word]
__global__ __launch_bounds__(BLOCK) void vox_scan_kernel(int tpc, const int32_t* __restrict__ tcnt, int32_t* __restrict__ toff, int32_t* __restrict__ cinfo, int word) {
    __shared__ int wsum[BLOCK / WAVE];
    const int b = blockIdx.x;
    const size_t q0 = (size_t)b * tpc;
    int run = 0;
    for (int t0 = 0; t0 < tpc; t0 += BLOCK) {
        const int t = t0 + threadIdx.x;
        int tot;
        const int pre = block_excl_scan<BLOCK>(t < tpc ? tcnt[q0 + t] : 0, wsum, tot);
        if (t < tpc) toff[q0 + t] = run + pre;
        run += tot;
    }
    if (threadIdx.x == 0) cinfo[(size_t)b * VOX_CI + word] = run;
}

template <int MODE>
__global__ __launch_bounds__(BLOCK) void vox_seg_write_kernel(int N, int m, int tpc, const int32_t* __restrict__ cinfo, const uint64_t* __restrict__ key0,
                                                              const uint64_t* __restrict__ key1, int32_t* __restrict__ start, int min_points,
                                                              const int32_t* __restrict__ toff, int32_t* __restrict__ vidof) {
    __shared__ int wsum[BLOCK / WAVE];
    int b, t;
    if (!vox_decode(tpc, N, b, t)) return;
    const int32_t* ci = cinfo + (size_t)b * VOX_CI;
    const int n = MODE == MODE_HEAD ? ci[CI_NV] : ci[CI_V];
    if (t * VOX_TILE >= n) return;                          // (block-uniform)
    const uint64_t* key = ((ci[CI_PASSES] & 1) ? key1 : key0) + (size_t)b * m;
    int32_t* st = start + (size_t)b * (m + 1);
    int32_t* vo = vidof + (size_t)b * m;
    int run = toff[(size_t)b * tpc + t];
    for (int k = 0; k < VOX_IPT; ++k) {
        const int i = t * VOX_TILE + k * BLOCK + threadIdx.x;
        const bool f = i < n && vox_flag<MODE>(i, key, st, min_points);
        int tot;
        const int id = run + block_flag_prefix(f, wsum, tot);
        if (f) {
            if (MODE == MODE_HEAD) {
                st[id] = i;
                if (min_points <= 1) vo[id] = id;
            } else {
                vo[id] = i;
            }
        }
        if (MODE == MODE_HEAD && i == n - 1) st[ci[CI_V]] = n;
        run += tot;
    }
}

// rows_out and the error word: ((first failing cloud + 1) << 2) | code, 0 when every cloud is fine
__global__ __launch_bounds__(BLOCK) void vox_finish_kernel(int N, int filtered, int32_t* __restrict__ cinfo, int32_t* __restrict__ rows_out) {
    __shared__ unsigned int first;
    if (threadIdx.x == 0) first = 0xffffffffu;
    __syncthreads();
    unsigned int e = 0xffffffffu;
    for (int b = threadIdx.x; b < N; b += BLOCK) {
        int32_t* ci = cinfo + (size_t)b * VOX_CI;
        const int r = ci[CI_ERR] ? 0 : (filtered ? ci[CI_OUT] : ci[CI_V]);
        ci[CI_OUT] = r;
        rows_out[b] = r;
        if (ci[CI_ERR]) e = min(e, ((unsigned int)(b + 1) << 2) | (unsigned int)ci[CI_ERR]);
    }
    atomicMin(&first, e);                                   // (an integer minimum: the same word whatever the order)
    __syncthreads();
    if (threadIdx.x == 0) rows_out[N] = first == 0xffffffffu ? 0 : (int32_t)first;
}

// ------------------------------------------------------------------ reduce
__global__ __launch_bounds__(BLOCK) void vox_fill_inverse_kernel(int64_t* __restrict__ inv, size_t n) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) inv[i] = -1;
}

struct VoxRef {            // one output voxel: its first sorted slot and row count, the cloud's sorted row indices
    int s0, cnt;
    const int32_t* idx;
};
__device__ __forceinline__ VoxRef vox_ref(int b, int o, int m, const int32_t* __restrict__ cinfo, const int32_t* __restrict__ start,
                                          const int32_t* __restrict__ vidof, const int32_t* __restrict__ idx0, const int32_t* __restrict__ idx1) {
    const int vid = vidof[(size_t)b * m + o];
    const int32_t* st = start + (size_t)b * (m + 1);
    VoxRef r;
    r.s0 = st[vid];
    r.cnt = st[vid + 1] - r.s0;
    r.idx = ((cinfo[(size_t)b * VOX_CI + CI_PASSES] & 1) ? idx1 : idx0) + (size_t)b * m;
    return r;
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void vox_reduce_small_kernel(const T* __restrict__ pts, int c, int N, int m, int M, int bpc, const int32_t* __restrict__ cinfo,
                                                                 const int32_t* __restrict__ start, const int32_t* __restrict__ vidof,
                                                                 const int32_t* __restrict__ idx0, const int32_t* __restrict__ idx1,
                                                                 T* __restrict__ cent, int32_t* __restrict__ counts, int64_t* __restrict__ inv,
                                                                 int32_t* __restrict__ big, int32_t* __restrict__ bigcount) {
    int b, blk;
    if (!vox_decode(bpc, N, b, blk)) return;
    const int o = blk * BLOCK + threadIdx.x;
    if (o >= min(cinfo[(size_t)b * VOX_CI + CI_OUT], M)) return;
    const VoxRef r = vox_ref(b, o, m, cinfo, start, vidof, idx0, idx1);
    counts[(size_t)b * M + o] = r.cnt;
    if (r.cnt > VOX_SMALL) {
        const int slot = atomicAdd(bigcount, 1);            // (an integer counter: which block takes a voxel never changes its sum)
        big[2 * slot] = b;
        big[2 * slot + 1] = o;
        return;
    }
    const T* P = pts + (size_t)b * m * c;
    T* out = cent + ((size_t)b * M + o) * c;
    for (int k = 0; k < r.cnt; ++k) inv[(size_t)b * m + r.idx[r.s0 + k]] = o;
    for (int j0 = 0; j0 < c; j0 += 4) {
        const int nj = min(4, c - j0);
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < r.cnt; ++k) {
            const T* p = P + (size_t)r.idx[r.s0 + k] * c + j0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nj) acc[j] += (double)p[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nj) out[j0 + j] = (T)(acc[j] / (double)r.cnt);
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void vox_reduce_big_kernel(const T* __restrict__ pts, int c, int m, int M, const int32_t* __restrict__ cinfo,
                                                               const int32_t* __restrict__ start, const int32_t* __restrict__ vidof,
                                                               const int32_t* __restrict__ idx0, const int32_t* __restrict__ idx1,
                                                               T* __restrict__ cent, int64_t* __restrict__ inv,
                                                               const int32_t* __restrict__ big, const int32_t* __restrict__ bigcount) {
    __shared__ double red[4][BLOCK];
    const int nbig = *bigcount;
    for (int q = blockIdx.x; q < nbig; q += gridDim.x) {
        const int b = big[2 * q], o = big[2 * q + 1];
        const VoxRef r = vox_ref(b, o, m, cinfo, start, vidof, idx0, idx1);
        const T* P = pts + (size_t)b * m * c;
        T* out = cent + ((size_t)b * M + o) * c;
        for (int k = threadIdx.x; k < r.cnt; k += BLOCK) inv[(size_t)b * m + r.idx[r.s0 + k]] = o;
        for (int j0 = 0; j0 < c; j0 += 4) {
            const int nj = min(4, c - j0);
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int k = threadIdx.x; k < r.cnt; k += BLOCK) {
                const T* p = P + (size_t)r.idx[r.s0 + k] * c + j0;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nj) acc[j] += (double)p[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) red[j][threadIdx.x] = acc[j];
            __syncthreads();
            for (int s = BLOCK / 2; s > 0; s >>= 1) {       // a fixed tree
                if (threadIdx.x < s) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + s];
                }
                __syncthreads();
            }
            if (threadIdx.x < nj) out[j0 + threadIdx.x] = (T)(red[threadIdx.x][0] / (double)r.cnt);
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------ backward
template <typename T>
__global__ __launch_bounds__(BLOCK) void vox_backward_kernel(const T* __restrict__ g, const int64_t* __restrict__ inv, const int32_t* __restrict__ counts,
                                                             int m, int M, int c, size_t rows_total, T* __restrict__ grad) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= rows_total) return;
    const size_t b = i / m;
    const int64_t o = inv[i];
    T* out = grad + i * c;
    if (o < 0 || o >= M) {
        for (int j = 0; j < c; ++j) out[j] = T(0);
        return;
    }
    const T n = (T)counts[b * M + o];
    const T* gi = g + (b * M + o) * c;
    for (int j = 0; j < c; ++j) out[j] = gi[j] / n;
}

int vox_check(int dtype, int N, int m, int c) {
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (N <= 0 || m <= 0 || c < 3 || N >= (1 << 29) || m >= 0x7fffffff - VOX_TILE) return DICP_ERR_SHAPE;
    return 0;
}

}  // namespace

size_t dicp_voxel_workspace_bytes(int dtype, int N, int m, int c) {
    if (vox_check(dtype, N, m, c)) return 0;
    return vox_layout(N, m).total;
}

int dicp_voxel_count(int dtype, const void* pts, int c, const int32_t* rows, int N, int m, double sx, double sy, double sz,
                     const void* origin, int origin_per_cloud, int min_points, int32_t* rows_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!pts || !rows_out || !workspace) return DICP_ERR_NULL;
    int rc = vox_check(dtype, N, m, c);
    if (rc) return rc;
    if ((origin_per_cloud != 0 && origin_per_cloud != 1) || min_points < 1) return DICP_ERR_SHAPE;
    if (!(sx > 0 && sy > 0 && sz > 0) || !(sx < HUGE_VAL && sy < HUGE_VAL && sz < HUGE_VAL)) return DICP_ERR_SHAPE;
    const VoxLayout L = vox_layout(N, m);
    if (workspace_bytes < L.total) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(pts, ts) || misaligned(origin, ts) || misaligned(rows_out, 4) || misaligned(rows, 4)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int tpc = vox_tiles(m);
    const unsigned g = vox_grid(N, tpc);
    const int os = origin_per_cloud ? 3 : 0;
    uint64_t* key[2] = {(uint64_t*)(ws + L.key[0]), (uint64_t*)(ws + L.key[1])};
    int32_t* idx[2] = {(int32_t*)(ws + L.idx[0]), (int32_t*)(ws + L.idx[1])};
    int32_t* start = (int32_t*)(ws + L.start);
    int32_t* vidof = (int32_t*)(ws + L.vidof);
    int64_t* tmin = (int64_t*)(ws + L.tmin);
    int64_t* tmax = (int64_t*)(ws + L.tmax);
    int32_t* tcnt = (int32_t*)(ws + L.tcnt);
    int32_t* tbad = (int32_t*)(ws + L.tbad);
    int32_t* toff = (int32_t*)(ws + L.toff);
    int32_t* hist = (int32_t*)(ws + L.hist);
    int32_t* cinfo = (int32_t*)(ws + L.cinfo);
    int64_t* vlo = (int64_t*)(ws + L.vlo);
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        const T s0 = (T)sx, s1 = (T)sy, s2 = (T)sz;
        vox_bounds_kernel<T><<<g, BLOCK, 0, st>>>((const T*)pts, c, rows, N, m, tpc, s0, s1, s2, (const T*)origin, os, tmin, tmax, tcnt, tbad);
        vox_plan_kernel<<<N, BLOCK, 0, st>>>(N, tpc, tmin, tmax, tcnt, tbad, toff, cinfo, vlo);
        vox_keys_kernel<T><<<g, BLOCK, 0, st>>>((const T*)pts, c, rows, N, m, tpc, s0, s1, s2, (const T*)origin, os, toff, cinfo, vlo, key[0], idx[0]);
    });
    for (int p = 0; p < VOX_MAX_PASSES; ++p) {              // a cloud that needs fewer passes leaves these launches at once
        vox_hist_kernel<<<g, BLOCK, 0, st>>>(N, m, tpc, p, cinfo, key[p & 1], hist);
        vox_digit_scan_kernel<<<N, VOX_SCAN_THREADS, 0, st>>>(tpc, p, cinfo, hist);
        vox_scatter_kernel<<<g, BLOCK, 0, st>>>(N, m, tpc, p, cinfo, hist, key[p & 1], idx[p & 1], key[(p + 1) & 1], idx[(p + 1) & 1]);
    }
    vox_seg_count_kernel<MODE_HEAD><<<g, BLOCK, 0, st>>>(N, m, tpc, cinfo, key[0], key[1], start, min_points, tcnt);
    vox_scan_kernel<<<N, BLOCK, 0, st>>>(tpc, tcnt, toff, cinfo, CI_V);
    vox_seg_write_kernel<MODE_HEAD><<<g, BLOCK, 0, st>>>(N, m, tpc, cinfo, key[0], key[1], start, min_points, toff, vidof);
    if (min_points > 1) {
        vox_seg_count_kernel<MODE_KEEP><<<g, BLOCK, 0, st>>>(N, m, tpc, cinfo, key[0], key[1], start, min_points, tcnt);
        vox_scan_kernel<<<N, BLOCK, 0, st>>>(tpc, tcnt, toff, cinfo, CI_OUT);
        vox_seg_write_kernel<MODE_KEEP><<<g, BLOCK, 0, st>>>(N, m, tpc, cinfo, key[0], key[1], start, min_points, toff, vidof);
    }
    vox_finish_kernel<<<1, BLOCK, 0, st>>>(N, min_points > 1, cinfo, rows_out);
    return launch_status();
}

int dicp_voxel_reduce(int dtype, const void* pts, int c, int N, int m, int M, const void* workspace, size_t workspace_bytes,
                      void* centroids, int32_t* counts, int64_t* inverse, void* stream) {
    if (!pts || !workspace || !inverse || (M > 0 && (!centroids || !counts))) return DICP_ERR_NULL;
    int rc = vox_check(dtype, N, m, c);
    if (rc) return rc;
    if (M < 0 || M > m) return DICP_ERR_SHAPE;
    const VoxLayout L = vox_layout(N, m);
    if (workspace_bytes < L.total) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(pts, ts) || misaligned(centroids, ts) || misaligned(counts, 4) || misaligned(inverse, 8)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const char* ws = (const char*)workspace;
    const size_t rows_total = (size_t)N * m;
    begin_launch();
    vox_fill_inverse_kernel<<<grid_1d(rows_total), BLOCK, 0, st>>>(inverse, rows_total);
    if ((rc = launch_status())) return rc;
    if (M == 0) return 0;
    if ((rc = dicp_fill::zero(centroids, (size_t)N * M * c * ts, st))) return rc;
    if ((rc = dicp_fill::zero(counts, (size_t)N * M * 4, st))) return rc;
    int32_t* bigcount = (int32_t*)(ws + L.bigcount);
    if ((rc = dicp_fill::zero(bigcount, 4, st))) return rc;
    const int32_t* cinfo = (const int32_t*)(ws + L.cinfo);
    const int32_t* start = (const int32_t*)(ws + L.start);
    const int32_t* vidof = (const int32_t*)(ws + L.vidof);
    const int32_t* idx0 = (const int32_t*)(ws + L.idx[0]);
    const int32_t* idx1 = (const int32_t*)(ws + L.idx[1]);
    int32_t* big = (int32_t*)(ws + L.big);
    const int bpc = (M + BLOCK - 1) / BLOCK;
    const unsigned g = vox_grid(N, bpc);
    const size_t cap = vox_big_cap(N, m);
    const unsigned gb = (unsigned)(cap < (size_t)VOX_BIG_BLOCKS ? cap : (size_t)VOX_BIG_BLOCKS);
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        vox_reduce_small_kernel<T><<<g, BLOCK, 0, st>>>((const T*)pts, c, N, m, M, bpc, cinfo, start, vidof, idx0, idx1, (T*)centroids, counts, inverse, big, bigcount);
        vox_reduce_big_kernel<T><<<gb, BLOCK, 0, st>>>((const T*)pts, c, m, M, cinfo, start, vidof, idx0, idx1, (T*)centroids, inverse, big, bigcount);
    });
    return launch_status();
}

int dicp_voxel_backward(int dtype, const void* grad_centroids, const int64_t* inverse, const int32_t* counts, int N, int m, int M, int c,
                        void* grad_pts, void* stream) {
    if (!inverse || !grad_pts || (M > 0 && (!grad_centroids || !counts))) return DICP_ERR_NULL;
    int rc = vox_check(dtype, N, m, c);
    if (rc) return rc;
    if (M < 0 || M > m) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(grad_centroids, ts) || misaligned(grad_pts, ts) || misaligned(counts, 4) || misaligned(inverse, 8)) return DICP_ERR_ALIGN;
    const size_t rows_total = (size_t)N * m;
    const unsigned g = (unsigned)((rows_total + BLOCK - 1) / BLOCK);
    begin_launch();
    if (dtype == DICP_F32) vox_backward_kernel<float><<<g, BLOCK, 0, (hipStream_t)stream>>>((const float*)grad_centroids, inverse, counts, m, M, c, rows_total, (float*)grad_pts);
    else                   vox_backward_kernel<double><<<g, BLOCK, 0, (hipStream_t)stream>>>((const double*)grad_centroids, inverse, counts, m, M, c, rows_total, (double*)grad_pts);
    return launch_status();
}
