// The inverted index of a neighbour index tensor (dicp_amd/group.py: invert_neighbors): per feature row, the flat numbers of the live slots
// that name it, in ascending order.  The rules per element are csrc/dicp_inverse.h's.
//
// A stable LSD radix sort of (key = the slot's row, or m for an empty slot; payload = the slot's flat number q), fed in ascending q, per
// cloud, 8 bits a pass over the ceil(bits(m) / 8) digits that hold a key -- two passes up to m = 65534.  Stable passes keep equal keys in
// the order they came in, so every row's list ascends in q by construction: no cursor, nothing to put in order afterwards, and the same
// cost whatever the in-degrees are (all n k slots on one row is one digit bucket like any other).  The pattern is voxel.hip's:
//   keys      flat over the slots: the 32-bit key of each
//   hist      per tile of INV_TILE slots (a tile never straddles two clouds): the digit histogram, integer LDS atomics (exact totals)
//   scan      per cloud (one workgroup): (digit, tile) -> the tile's first output position per digit
//   scatter   per tile: rounds of 256 slots in order, each ranked within its wave by 8 ballots and across the waves through LDS counts;
//             the last pass writes the payloads straight into `slots`, -1 for an empty slot
//   offsets   flat over the sorted positions: a position whose key differs from its predecessor's writes the offsets of the rows between
//             the two keys, so offsets (N, m + 1) is written once per element from the sorted keys, without a count or a zero fill
// Workspace: two key and two payload arrays of n k int32 and the tile histograms, O(n k) per cloud.  Nothing is read back.
//
// The deterministic backward into a feature table (dicp_*_backward_det) is a gather over that index instead of group.hip's scatter:
// det_bwd_kernel gives every lane one pack of one DESTINATION row and walks the row's list (csrc/dicp_inverse.h has the walk and its order
// of summation), so every element of grad_features is stored once -- no zero fill, no float atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_group.h"
#include "dicp_group_launch.h"
#include "dicp_inverse.h"

namespace {

constexpr int INV_IPT = 16;                         // slots per thread and tile
constexpr int INV_TILE = BLOCK * INV_IPT;           // 4096 slots
constexpr int INV_SCAN_THREADS = 1024;              // the digit scan: 4 groups of tiles x 256 digits
static_assert(BLOCK == 256, "one thread per digit");

inline size_t inv_tiles(size_t nk) { return (nk + INV_TILE - 1) / INV_TILE; }

struct InvLayout { size_t key[2], pay[2], hist, total; };
inline InvLayout inv_layout(int N, size_t nk) {
    InvLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
    for (int i = 0; i < 2; ++i) L.key[i] = take((size_t)N * nk * 4);
    for (int i = 0; i < 2; ++i) L.pay[i] = take((size_t)N * nk * 4);
    L.hist = take((size_t)N * inv_tiles(nk) * 256 * 4);
    L.total = o;
    return L;
}

// N, n, m >= 1, 1 <= k <= GROUP_K_MAX, n k < 2^31 per cloud, one workgroup per (cloud, tile) in a grid, the batch's bytes below 2^62
inline bool inv_shape_ok(int N, int n, int m, int k) {
    if (N < 1 || n < 1 || m < 1 || k < 1 || k > GROUP_K_MAX) return false;
    const size_t nk = (size_t)n * k;
    if (nk >= ((size_t)1 << 31)) return false;
    if ((size_t)N * inv_tiles(nk) >= ((size_t)1 << 31)) return false;
    return (size_t)N <= (((size_t)1 << 58) / (nk + 1)) && (size_t)N <= (((size_t)1 << 58) / ((size_t)m + 1));
}

template <typename I>
__global__ __launch_bounds__(BLOCK) void inv_keys_kernel(const I* __restrict__ idx, const int32_t* __restrict__ rows, size_t total, size_t nk, int m, uint32_t* __restrict__ key) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLOCK)
        key[i] = inverse_key(group_row(idx[i], rows_of(rows, (int)(i / nk), m)), m);
}

__global__ __launch_bounds__(BLOCK) void inv_hist_kernel(size_t nk, unsigned tpc, int shift, const uint32_t* __restrict__ key, int32_t* __restrict__ hist) {
    __shared__ int h[256];
    const size_t b = blockIdx.x / tpc, t = blockIdx.x % tpc;
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t* K = key + b * nk;
    for (int r = 0; r < INV_IPT; ++r) {
        const size_t i = t * INV_TILE + (size_t)r * BLOCK + threadIdx.x;
        if (i < nk) atomicAdd(&h[(K[i] >> shift) & 255u], 1);
    }
    __syncthreads();
    hist[(size_t)blockIdx.x * 256 + threadIdx.x] = h[threadIdx.x];
}

// exclusive prefix of v over the workgroup's threads in thread order.  lds: NT / 64 ints
template <int NT>
__device__ __forceinline__ int inv_block_scan(int v, int* lds) {
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    int x = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == WAVE - 1) lds[w] = x;
    __syncthreads();
    int pre = 0;
#pragma unroll
    for (int q = 0; q < NT / WAVE; ++q) pre += q < w ? lds[q] : 0;
    return pre + x - v;
}

// hist (N, tpc, 256) counts -> each tile's first position per digit within its cloud (in place): digit-major, tile-minor
__global__ __launch_bounds__(INV_SCAN_THREADS) void inv_digit_scan_kernel(unsigned tpc, int32_t* __restrict__ hist) {
    constexpr int G = INV_SCAN_THREADS / 256;
    __shared__ int part[G][256];
    __shared__ int wsum[INV_SCAN_THREADS / WAVE];
    __shared__ int bases[256];
    const unsigned g = threadIdx.x / 256, d = threadIdx.x % 256;
    const unsigned chunk = (tpc + G - 1) / G, t0 = min(g * chunk, tpc), t1 = min(t0 + chunk, tpc);
    int32_t* H = hist + (size_t)blockIdx.x * tpc * 256;
    int s = 0;
    for (unsigned t = t0; t < t1; ++t) s += H[(size_t)t * 256 + d];
    part[g][d] = s;
    __syncthreads();
    int total = 0, pre = 0;
#pragma unroll
    for (unsigned q = 0; q < G; ++q) { const int x = part[q][d]; pre += q < g ? x : 0; total += x; }
    const int dbase = inv_block_scan<INV_SCAN_THREADS>(g == 0 ? total : 0, wsum);     // (threads of g = 0 first: digit order)
    if (g == 0) bases[d] = dbase;
    __syncthreads();
    int run = bases[d] + pre;
    for (unsigned t = t0; t < t1; ++t) {
        const int x = H[(size_t)t * 256 + d];
        H[(size_t)t * 256 + d] = run;
        run += x;
    }
}

// stable scatter of one digit.  pay_in = NULL: the payload is the position itself (the first pass).  dead >= 0: the last pass, the
// payload of a slot with key `dead` (an empty slot) is written as -1.  Every output position is below n k: the bases are the scan of
// this cloud's own histograms.
__global__ __launch_bounds__(BLOCK) void inv_scatter_kernel(size_t nk, unsigned tpc, int shift, const int32_t* __restrict__ hist, const uint32_t* __restrict__ key_in,
                                                            const int32_t* __restrict__ pay_in, uint32_t* __restrict__ key_out, int32_t* __restrict__ pay_out, int64_t dead) {
    constexpr int NW = BLOCK / WAVE;
    __shared__ int dbase[256];
    __shared__ int wcnt[NW][256];
    const size_t b = blockIdx.x / tpc, t = blockIdx.x % tpc;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    dbase[threadIdx.x] = hist[(size_t)blockIdx.x * 256 + threadIdx.x];
#pragma unroll
    for (int q = 0; q < NW; ++q) wcnt[q][threadIdx.x] = 0;
    __syncthreads();
    const size_t base = b * nk;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int r = 0; r < INV_IPT; ++r) {                     // (workgroup-uniform trips: the barriers)
        const size_t i = t * INV_TILE + (size_t)r * BLOCK + threadIdx.x;
        const bool act = i < nk;
        uint32_t kk = 0;
        int32_t id = 0;
        if (act) { kk = key_in[base + i]; id = pay_in ? pay_in[base + i] : (int32_t)i; }
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
            if ((size_t)pos < nk) {                         // (always: see above)
                key_out[base + pos] = kk;
                pay_out[base + pos] = (int64_t)kk == dead ? -1 : id;
            }
        }
        __syncthreads();
        int s = 0;
#pragma unroll
        for (int q = 0; q < NW; ++q) { s += wcnt[q][threadIdx.x]; wcnt[q][threadIdx.x] = 0; }
        dbase[threadIdx.x] += s;
        __syncthreads();
    }
}

// offsets (N, m + 1) from the sorted keys: one item per sorted position and one past the end, per cloud
__global__ __launch_bounds__(BLOCK) void inv_offsets_kernel(const uint32_t* __restrict__ key, size_t total, size_t nk, int m, int32_t* __restrict__ offsets) {
    for (size_t it = (size_t)blockIdx.x * BLOCK + threadIdx.x; it < total; it += (size_t)gridDim.x * BLOCK) {
        const size_t b = it / (nk + 1);
        const int64_t p = (int64_t)(it - b * (nk + 1));
        int64_t first, last;
        inverse_offset_rows(key + b * nk, p, (int64_t)nk, m, first, last);
        if (last > m) last = m;                             // (a key is at most m)
        int32_t* O = offsets + b * ((size_t)m + 1);
        for (int64_t j = first; j <= last; ++j) O[j] = (int32_t)p;
    }
}

// ------------------------------------------------------------------ the deterministic backward into the features
// One lane per (destination row, pack of V channels), consecutive lanes consecutive packs of a row: the store and the cotangent loads of
// the lanes of a row are contiguous segments.  V = 16 bytes of channels where C * sizeof(T) and the bases are multiples of 16 (the wide
// form: a row of C = 64 float32 is 16 lanes), V = 1 otherwise (the narrow form, lanes over (row, channel): C = 1, 3, 33, 65, 130, a
// misaligned view).  A lane walks its row's list sequentially (dicp_inverse.h: det_row_sum); the lanes of a row read the same entries, one
// broadcast load each.  The walk is bounded by the list's clamps and its entry check whatever offsets / slots hold.
template <typename T, typename I, int V, int OP>
__global__ __launch_bounds__(BLOCK) void det_bwd_kernel(DetCloud<T, I> a, const int32_t* __restrict__ rows, const int32_t* __restrict__ offsets, const int32_t* __restrict__ slots,
                                                        size_t total, int m, T* __restrict__ gf) {
    const int VR = a.C / V;
    const size_t nk = (size_t)a.n * a.k, qc = (size_t)a.n * a.C;
    for (size_t it = (size_t)blockIdx.x * BLOCK + threadIdx.x; it < total; it += (size_t)gridDim.x * BLOCK) {
        const size_t row = it / VR;
        const int c = (int)(it - row * VR) * V;
        const size_t b = row / m;
        const int j = (int)(row - b * m);
        DetCloud<T, I> cl = a;                              // cloud b's arrays
        cl.g = a.g + b * (OP == DET_GROUP ? nk * a.C : qc);
        cl.idx = a.idx + b * nk;
        if (OP == DET_POOL_MAX) cl.argmax = a.argmax + b * qc;
        if (OP == DET_POOL_MEAN) cl.counts = a.counts + b * a.n;
        if (OP == DET_INTERP) cl.d2 = a.d2 + b * nk;
        cl.rows = rows_of(rows, (int)b, m);
        Pack<T, V> x;
        det_row_sum<T, I, V, OP>(cl, offsets + b * ((size_t)m + 1), slots + b * nk, j, c, x.v);
        pack_store<T, V>(gf + row * a.C + c, x);
    }
}

// the checks the three deterministic entry points share, after their own null and enum checks
int det_check(int dtype, int idx64, int N, int n, int m, int k, int C) {
    int rc = group_check(dtype, idx64, N, n, m, k, C);
    if (rc) return rc;
    if ((size_t)n * k >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;       // a cloud's slot numbers are int32
    return 0;
}

// det_bwd_kernel<T, I, V, OP> over the (N, m, C) table: 16-byte packs where the row size and both bases allow
template <int OP, typename T, typename I>
void det_launch(DetCloud<T, I> a, int dtype, const int32_t* rows, const int32_t* offsets, const int32_t* slots, int N, int m, void* gf, hipStream_t st) {
    constexpr int V = VecOf<T>::v;
    if (vec16(dtype, a.C, a.g, gf)) {
        const size_t total = (size_t)N * m * (a.C / V);
        det_bwd_kernel<T, I, V, OP><<<group_grid(total, BLOCK), BLOCK, 0, st>>>(a, rows, offsets, slots, total, m, (T*)gf);
    } else {
        const size_t total = (size_t)N * m * a.C;
        det_bwd_kernel<T, I, 1, OP><<<group_grid(total, BLOCK), BLOCK, 0, st>>>(a, rows, offsets, slots, total, m, (T*)gf);
    }
}

}  // namespace

size_t dicp_invert_neighbors_workspace_bytes(int N, int n, int m, int k) {
    if (!inv_shape_ok(N, n, m, k)) return 0;
    return inv_layout(N, (size_t)n * k).total;
}

int dicp_invert_neighbors(const void* idx, int idx64, const int32_t* rows, int N, int n, int m, int k,
                          int32_t* offsets, int32_t* slots, void* workspace, size_t workspace_bytes, void* stream) {
    if (!idx || !offsets || !slots || !workspace) return DICP_ERR_NULL;
    if (idx64 != 0 && idx64 != 1) return DICP_ERR_ENUM;
    if (!inv_shape_ok(N, n, m, k)) return DICP_ERR_SHAPE;
    const size_t nk = (size_t)n * k;
    const InvLayout L = inv_layout(N, nk);
    if (workspace_bytes < L.total) return DICP_ERR_SHAPE;
    if (misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4) || misaligned(offsets, 4) || misaligned(slots, 4) || misaligned(workspace, 256)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint32_t* key[2] = {(uint32_t*)(ws + L.key[0]), (uint32_t*)(ws + L.key[1])};
    int32_t* pay[2] = {(int32_t*)(ws + L.pay[0]), (int32_t*)(ws + L.pay[1])};
    int32_t* hist = (int32_t*)(ws + L.hist);
    const unsigned tpc = (unsigned)inv_tiles(nk), tiles = (unsigned)N * tpc;
    const size_t total = (size_t)N * nk;
    const int passes = inverse_passes(m);
    begin_launch();
    if (idx64) inv_keys_kernel<int64_t><<<grid_1d(total), BLOCK, 0, st>>>((const int64_t*)idx, rows, total, nk, m, key[0]);
    else       inv_keys_kernel<int32_t><<<grid_1d(total), BLOCK, 0, st>>>((const int32_t*)idx, rows, total, nk, m, key[0]);
    for (int p = 0; p < passes; ++p) {
        const bool last = p == passes - 1;
        inv_hist_kernel<<<tiles, BLOCK, 0, st>>>(nk, tpc, 8 * p, key[p & 1], hist);
        inv_digit_scan_kernel<<<(unsigned)N, INV_SCAN_THREADS, 0, st>>>(tpc, hist);
        inv_scatter_kernel<<<tiles, BLOCK, 0, st>>>(nk, tpc, 8 * p, hist, key[p & 1], p ? pay[(p - 1) & 1] : nullptr, key[(p + 1) & 1], last ? slots : pay[p & 1],
                                                    last ? (int64_t)m : (int64_t)-1);
    }
    inv_offsets_kernel<<<grid_1d((size_t)N * (nk + 1)), BLOCK, 0, st>>>(key[passes & 1], (size_t)N * (nk + 1), nk, m, offsets);
    return launch_status();
}

int dicp_group_backward_det(int dtype, const void* grad_out, const void* idx, int idx64, const int32_t* rows, int N, int n, int m, int k, int C,
                            const int32_t* offsets, const int32_t* slots, void* grad_features, void* stream) {
    if (!grad_out || !idx || !offsets || !slots || !grad_features) return DICP_ERR_NULL;
    int rc = det_check(dtype, idx64, N, n, m, k, C);
    if (rc) return rc;
    const size_t ts = elem_size(dtype);
    if (misaligned(grad_out, ts) || misaligned(grad_features, ts) || misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4) || misaligned(offsets, 4) || misaligned(slots, 4)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    begin_launch();
    with_scalar_index(dtype, idx64, [&](auto t, auto i) {
        using T = decltype(t);
        using I = decltype(i);
        const DetCloud<T, I> a = {(const T*)grad_out, (const I*)idx, nullptr, nullptr, nullptr, T(0), n, k, C, 0};
        det_launch<DET_GROUP>(a, dtype, rows, offsets, slots, N, m, grad_features, st);
    });
    return launch_status();
}

int dicp_pool_backward_det(int dtype, const void* grad_out, const void* idx, int idx64, const int32_t* rows, int reduce, const int32_t* argmax, const int32_t* counts,
                           int N, int n, int m, int k, int C, const int32_t* offsets, const int32_t* slots, void* grad_features, void* stream) {
    if (!grad_out || !idx || !offsets || !slots || !grad_features) return DICP_ERR_NULL;
    if (reduce != DICP_POOL_SUM && reduce != DICP_POOL_MEAN && reduce != DICP_POOL_MAX) return DICP_ERR_ENUM;
    if ((reduce == DICP_POOL_MAX && !argmax) || (reduce == DICP_POOL_MEAN && !counts)) return DICP_ERR_NULL;
    if (reduce != DICP_POOL_MAX && argmax) return DICP_ERR_ENUM;
    int rc = det_check(dtype, idx64, N, n, m, k, C);
    if (rc) return rc;
    const size_t ts = elem_size(dtype);
    if (misaligned(grad_out, ts) || misaligned(grad_features, ts) || misaligned(argmax, 4) || misaligned(counts, 4) || misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4)
        || misaligned(offsets, 4) || misaligned(slots, 4)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    begin_launch();
    with_scalar_index(dtype, idx64, [&](auto t, auto i) {
        using T = decltype(t);
        using I = decltype(i);
        const DetCloud<T, I> a = {(const T*)grad_out, (const I*)idx, argmax, counts, nullptr, T(0), n, k, C, 0};
        if (reduce == DICP_POOL_MAX)       det_launch<DET_POOL_MAX>(a, dtype, rows, offsets, slots, N, m, grad_features, st);
        else if (reduce == DICP_POOL_MEAN) det_launch<DET_POOL_MEAN>(a, dtype, rows, offsets, slots, N, m, grad_features, st);
        else                               det_launch<DET_POOL_SUM>(a, dtype, rows, offsets, slots, N, m, grad_features, st);
    });
    return launch_status();
}

int dicp_interpolate_backward_det(int dtype, const void* grad_out, const void* idx, int idx64, const int32_t* rows, const void* d2, double eps,
                                  int N, int n, int m, int k, int C, const int32_t* offsets, const int32_t* slots, void* grad_features, void* stream) {
    if (!grad_out || !idx || !d2 || !offsets || !slots || !grad_features) return DICP_ERR_NULL;
    int rc = det_check(dtype, idx64, N, n, m, k, C);
    if (rc) return rc;
    if (!(eps > 0.0) || eps - eps != 0.0) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(grad_out, ts) || misaligned(grad_features, ts) || misaligned(d2, ts) || misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4) || misaligned(offsets, 4)
        || misaligned(slots, 4)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    begin_launch();
    with_scalar_index(dtype, idx64, [&](auto t, auto i) {
        using T = decltype(t);
        using I = decltype(i);
        const DetCloud<T, I> a = {(const T*)grad_out, (const I*)idx, nullptr, nullptr, (const T*)d2, (T)eps, n, k, C, 0};
        det_launch<DET_INTERP>(a, dtype, rows, offsets, slots, N, m, grad_features, st);
    });
    return launch_status();
}
