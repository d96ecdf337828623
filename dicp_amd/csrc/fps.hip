// Farthest-point sampling of batches of clouds (dicp_amd/fps.py): k well-spread rows per cloud, the rule in csrc/dicp_fps.h.
//
// Resident form (clouds of up to FPS_THREADS * R rows): ONE workgroup of FPS_THREADS threads per cloud, for the whole call.  Thread t keeps
// rows t, t + FPS_THREADS, ... (x, y, z, D) in registers.  A step: every thread updates its R rows against the pick and keeps its best live
// row (key and coordinates: a select per row -- picking the coordinates afterwards by a register index sent the arrays to scratch); the wave
// reduces the key by shuffles; the lane that owns the wave's best row writes the key AND the row's coordinates to the wave's LDS slot (two
// sets of slots, by step parity); one barrier; every thread reduces the 16 slots and reads the winner's coordinates.  Nothing but the pick's
// index and distance (one lane) goes to memory inside the loop.
// Streamed form (larger clouds): (x, y, z, D) rows in a workspace, one launch per step over all clouds, FPS_STREAM_ROWS rows per workgroup.
// A workgroup writes its best key to its slot of the cloud (two sets, by parity); the prologue of the next launch reduces the cloud's slots in
// every workgroup.  A step's dependency on the one before is the kernel boundary: no grid barrier, no waiting on another workgroup.
// Both forms: picks' indices / distances / k_eff written as they are made, then one gather kernel writes the c output columns.
// Backward: a zero fill (dicp_fill.h) and a scatter of the cotangent's rows; indices are distinct per cloud, so no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_fill.h"
#include "dicp_fps.h"

namespace {

constexpr int FPS_THREADS = 1024;                  // the resident workgroup: 16 waves, 4 per SIMD -> 128 VGPRs a lane
constexpr int FPS_WAVES = FPS_THREADS / WAVE;
constexpr int FPS_R32 = 16, FPS_R64 = 8;           // rows per thread: 4 R registers of state (float32) / 8 R (float64) = 64 VGPRs
constexpr int FPS_STREAM_IPT = 8;
constexpr int FPS_STREAM_ROWS = BLOCK * FPS_STREAM_IPT;     // rows per workgroup of the streamed form

template <typename T> struct FpsR;
template <> struct FpsR<float>  { static constexpr int v = FPS_R32; };
template <> struct FpsR<double> { static constexpr int v = FPS_R64; };

inline int fps_resident_rows(int dtype) { return FPS_THREADS * (dtype == DICP_F32 ? FPS_R32 : FPS_R64); }
inline int fps_groups(int n) { return (n + FPS_STREAM_ROWS - 1) / FPS_STREAM_ROWS; }

__device__ __forceinline__ FpsKey<float> key_shfl_xor(const FpsKey<float>& a, int off) {
    FpsKey<float> r;
    r.k = __shfl_xor((unsigned long long)a.k, off);
    return r;
}
__device__ __forceinline__ FpsKey<double> key_shfl_xor(const FpsKey<double>& a, int off) {
    FpsKey<double> r;
    r.hi = __shfl_xor((unsigned long long)a.hi, off);
    r.lo = __shfl_xor(a.lo, off);
    r.pad = 0;
    return r;
}
template <typename T>
__device__ __forceinline__ FpsKey<T> key_max(const FpsKey<T>& a, const FpsKey<T>& b) { return fps_key_better(b, a) ? b : a; }

// the best key of the lanes whose numbers differ in the bits below `width` (a power of two <= 64), in every one of them
template <typename T>
__device__ __forceinline__ FpsKey<T> key_reduce(FpsKey<T> k, int width) {
    for (int off = 1; off < width; off <<= 1) k = key_max(k, key_shfl_xor(k, off));
    return k;
}

// start mod rows of cloud b (0 for an empty cloud)
__device__ __forceinline__ int fps_start(const int64_t* __restrict__ start, int b, int nb) {
    if (!start || nb <= 0) return 0;
    const int64_t s = start[b] % (int64_t)nb;
    return (int)(s < 0 ? s + nb : s);
}

// what one lane records of pick t: its index and distance, and the cloud's count so far
template <typename T>
__device__ __forceinline__ void fps_record(const FpsKey<T>& key, int t, int k, int b, int64_t* __restrict__ idx, T* __restrict__ dist, int32_t* __restrict__ keff) {
    const size_t o = (size_t)b * k + t;
    if (fps_key_empty(key)) {
        idx[o] = -1;
        dist[o] = inf_v<T>();
    } else {
        idx[o] = fps_key_index(key);
        dist[o] = t == 0 ? inf_v<T>() : fps_key_D(key);
        keff[b] = t + 1;
    }
}

// ------------------------------------------------------------------ resident form
template <typename T>
struct FpsSlot {               // one wave's best row of a step
    FpsKey<T> key;
    T x, y, z, pad;
};

// The waves' exchange: the wave's best key reduced over its lanes, published with its coordinates by the owning lane, then (after the
// step's one barrier) the workgroup's best key and coordinates in every thread.
template <typename T>
__device__ __forceinline__ FpsKey<T> fps_exchange(FpsKey<T> mine, T bx, T by, T bz, FpsSlot<T>* slots, T& px, T& py, T& pz) {
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const FpsKey<T> wk = key_reduce(mine, WAVE);
    if (fps_key_empty(wk) ? lane == 0 : (fps_key_index(wk) & (FPS_THREADS - 1)) == (int)threadIdx.x) {
        FpsSlot<T> s;
        s.key = wk; s.x = bx; s.y = by; s.z = bz; s.pad = T(0);
        slots[w] = s;
    }
    __syncthreads();
    FpsKey<T> best = key_reduce(slots[lane & (FPS_WAVES - 1)].key, FPS_WAVES);
    if (!fps_key_empty(best)) {
        const int ow = (fps_key_index(best) & (FPS_THREADS - 1)) / WAVE;
        px = slots[ow].x; py = slots[ow].y; pz = slots[ow].z;
    }
    return best;
}

template <typename T, int R>
__global__ __launch_bounds__(FPS_THREADS) void fps_resident_kernel(const T* __restrict__ pts, int c, const int32_t* __restrict__ rows, const int64_t* __restrict__ start,
                                                                   int n, int k, int64_t* __restrict__ idx, T* __restrict__ dist, int32_t* __restrict__ keff) {
    __shared__ FpsSlot<T> slots[2][FPS_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nb = rows_of(rows, b, n);
    const int st = fps_start(start, b, nb);
    const T* P = pts + (size_t)b * n * c;
    T x[R], y[R], z[R], D[R];
    FpsKey<T> mine = fps_key_none(T(0));
    T bx = T(0), by = T(0), bz = T(0);                      // the coordinates of the thread's best row
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = r * FPS_THREADS + tid;
        x[r] = y[r] = z[r] = T(0);
        D[r] = fps_picked<T>();
        if (row < nb) {
            const T* p = P + (size_t)row * c;
            const T a0 = p[0], a1 = p[1], a2 = p[2];
            if (fps_candidate(row, nb, a0, a1, a2)) {
                x[r] = a0; y[r] = a1; z[r] = a2;
                D[r] = inf_v<T>();
                const FpsKey<T> kr = fps_key_first(T(0), fps_rank(row, st, nb), row);
                if (fps_key_better(kr, mine)) { mine = kr; bx = a0; by = a1; bz = a2; }
            }
        }
    }
    if (tid == 0) keff[b] = 0;
    T px = T(0), py = T(0), pz = T(0);
    int t = 0;
    for (; t < k; ++t) {
        const FpsKey<T> best = fps_exchange<T>(mine, bx, by, bz, slots[t & 1], px, py, pz);
        if (fps_key_empty(best)) break;                     // (workgroup-uniform) no live row is left
        if (tid == 0) fps_record<T>(best, t, k, b, idx, dist, keff);
        if (t + 1 == k) { ++t; break; }
        const int jp = fps_key_index(best);
        T bd = fps_picked<T>();
        int bj = -1;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = r * FPS_THREADS + tid;
            const T d = fps_d2<T>(x[r], y[r], z[r], px, py, pz);
            T Dn = fps_update<T>(D[r], d);
            Dn = row == jp ? fps_picked<T>() : Dn;
            D[r] = Dn;
            if (fps_before<T>(Dn, row, bd, bj)) { bd = Dn; bj = row; bx = x[r]; by = y[r]; bz = z[r]; }
        }
        mine = fps_key_live<T>(bd, bj);
    }
    for (int s = t + tid; s < k; s += FPS_THREADS) {        // the unused slots
        idx[(size_t)b * k + s] = -1;
        dist[(size_t)b * k + s] = inf_v<T>();
    }
}

// ------------------------------------------------------------------ streamed form
// pts (N,n,c) -> rows4 (N,n,4): x, y, z and D = +inf for a candidate, the sentinel (and zero coordinates) otherwise
template <typename T>
__global__ __launch_bounds__(BLOCK) void fps_pack_kernel(const T* __restrict__ pts, int c, const int32_t* __restrict__ rows, int n, size_t total,
                                                         typename V4<T>::type* __restrict__ rows4, int32_t* __restrict__ keff, int N) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < (size_t)N) keff[i] = 0;
    if (i >= total) return;
    const int b = (int)(i / n), row = (int)(i - (size_t)b * n);
    const int nb = rows_of(rows, b, n);
    typename V4<T>::type v;
    v.x = v.y = v.z = T(0);
    v.w = fps_picked<T>();
    if (row < nb) {
        const T* p = pts + i * c;
        const T a0 = p[0], a1 = p[1], a2 = p[2];
        if (fps_candidate(row, nb, a0, a1, a2)) { v.x = a0; v.y = a1; v.z = a2; v.w = inf_v<T>(); }
    }
    rows4[i] = v;
}

// the workgroup's best key in every thread.  lds: BLOCK / WAVE keys; two barriers
template <typename T>
__device__ __forceinline__ FpsKey<T> fps_block_best(FpsKey<T> mine, FpsKey<T>* lds) {
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const FpsKey<T> wk = key_reduce(mine, WAVE);
    __syncthreads();                                        // (lds may still be read from the call before)
    if (lane == 0) lds[w] = wk;
    __syncthreads();
    return key_reduce(lds[lane & (BLOCK / WAVE - 1)], BLOCK / WAVE);
}

// launch s of k + 1: the prologue makes pick s - 1 from the slots of launch s - 1 and records it, the body updates the workgroup's rows
// against it and leaves the workgroup's best key in its slot for launch s + 1.  Launch 0 has no prologue (its keys are the ranks of
// pick 0), launch k no body.
template <typename T>
__global__ __launch_bounds__(BLOCK) void fps_stream_kernel(typename V4<T>::type* __restrict__ rows4, const int32_t* __restrict__ rows, const int64_t* __restrict__ start,
                                                           int N, int n, int G, int s, int k, FpsKey<T>* __restrict__ slots,
                                                           int64_t* __restrict__ idx, T* __restrict__ dist, int32_t* __restrict__ keff) {
    __shared__ FpsKey<T> lds[BLOCK / WAVE];
    const int b = blockIdx.x / G, g = blockIdx.x - b * G, tid = threadIdx.x;
    const int nb = rows_of(rows, b, n);
    typename V4<T>::type* R4 = rows4 + (size_t)b * n;
    FpsKey<T>* mine_slot = slots + ((size_t)(s & 1) * N + b) * G + g;
    int jp = -1;
    T px = T(0), py = T(0), pz = T(0);
    if (s > 0) {
        const FpsKey<T>* prev = slots + ((size_t)((s - 1) & 1) * N + b) * G;
        FpsKey<T> best = fps_key_none(T(0));
        for (int i = tid; i < G; i += BLOCK) best = key_max(best, prev[i]);
        best = fps_block_best<T>(best, lds);
        if (g == 0 && tid == 0) fps_record<T>(best, s - 1, k, b, idx, dist, keff);
        if (fps_key_empty(best) || s == k) {                // (workgroup-uniform) the cloud is finished: later launches find an empty key
            if (s < k && tid == 0) *mine_slot = fps_key_none(T(0));
            return;
        }
        jp = fps_key_index(best);
        const T* pj = (const T*)(R4 + jp);                  // (x, y, z only: the row's D is being written by the workgroup that owns it)
        px = pj[0]; py = pj[1]; pz = pj[2];
    }
    const int st = fps_start(start, b, nb);
    FpsKey<T> mine = fps_key_none(T(0));
    for (int i = 0; i < FPS_STREAM_IPT; ++i) {
        const int row = g * FPS_STREAM_ROWS + i * BLOCK + tid;
        if (row >= nb) break;                               // (rows at or past nb hold the sentinel: nothing to update)
        const typename V4<T>::type v = R4[row];
        if (s == 0) {
            if (v.w >= T(0)) mine = key_max(mine, fps_key_first(T(0), fps_rank(row, st, nb), row));
        } else {
            const T d = fps_d2<T>(v.x, v.y, v.z, px, py, pz);
            T Dn = fps_update<T>(v.w, d);
            Dn = row == jp ? fps_picked<T>() : Dn;
            if (Dn != v.w) R4[row].w = Dn;
            mine = key_max(mine, fps_key_live<T>(Dn, row));
        }
    }
    mine = fps_block_best<T>(mine, lds);
    if (tid == 0) *mine_slot = mine;
}

// ------------------------------------------------------------------ gather / scatter
// out (N,k,c) = pts[b, idx[b, s]] (zero rows where idx = -1)
template <typename T>
__global__ __launch_bounds__(BLOCK) void fps_gather_kernel(const T* __restrict__ pts, const int64_t* __restrict__ idx, int n, int k, int c, size_t total, T* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= total) return;
    const size_t slot = i / c;
    const int col = (int)(i - slot * c);
    const size_t b = slot / k;
    const int64_t j = idx[slot];
    out[i] = (j >= 0 && j < n) ? pts[(b * n + (size_t)j) * c + col] : T(0);
}

// grad (N,n,c), zeroed: grad[b, idx[b, s]] = g[b, s]
template <typename T>
__global__ __launch_bounds__(BLOCK) void fps_scatter_kernel(const T* __restrict__ g, const int64_t* __restrict__ idx, int n, int k, int c, size_t total, T* __restrict__ grad) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= total) return;
    const size_t slot = i / c;
    const int col = (int)(i - slot * c);
    const size_t b = slot / k;
    const int64_t j = idx[slot];
    if (j >= 0 && j < n) grad[(b * n + (size_t)j) * c + col] = g[i];
}

int fps_check(int dtype, int N, int n, int k, int c) {
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (N < 1 || n < 1 || k < 1 || c < 3 || n >= 0x7fffffff - FPS_STREAM_ROWS || (size_t)N * (size_t)fps_groups(n) >= 0x7fffffffu) return DICP_ERR_SHAPE;
    return 0;
}

bool fps_streamed(int dtype, int n, int form) { return form == DICP_FPS_STREAMED || (form == DICP_FPS_AUTO && n > fps_resident_rows(dtype)); }

struct FpsLayout { size_t rows4, slots, total; };
inline FpsLayout fps_layout(int dtype, int N, int n) {
    const size_t ts = elem_size(dtype), ks = dtype == DICP_F32 ? sizeof(FpsKey<float>) : sizeof(FpsKey<double>);
    FpsLayout L;
    L.rows4 = 0;
    L.slots = up256((size_t)N * n * 4 * ts);
    L.total = up256(L.slots + 2 * (size_t)N * fps_groups(n) * ks);
    return L;
}

template <typename T, int R>
void fps_launch_resident(const void* pts, int c, const int32_t* rows, const int64_t* start, int N, int n, int k, int64_t* idx, void* dist, int32_t* keff, hipStream_t st) {
    fps_resident_kernel<T, R><<<N, FPS_THREADS, 0, st>>>((const T*)pts, c, rows, start, n, k, idx, (T*)dist, keff);
}

// the smallest instantiation that holds n rows: a short cloud does not pay for 16 rows a thread
template <typename T>
void fps_resident(const void* pts, int c, const int32_t* rows, const int64_t* start, int N, int n, int k, int64_t* idx, void* dist, int32_t* keff, hipStream_t st) {
    const int need = (n + FPS_THREADS - 1) / FPS_THREADS;
    if (need <= 1)      fps_launch_resident<T, 1>(pts, c, rows, start, N, n, k, idx, dist, keff, st);
    else if (need <= 2) fps_launch_resident<T, 2>(pts, c, rows, start, N, n, k, idx, dist, keff, st);
    else if (need <= 4) fps_launch_resident<T, 4>(pts, c, rows, start, N, n, k, idx, dist, keff, st);
    else if (need <= 8) fps_launch_resident<T, 8>(pts, c, rows, start, N, n, k, idx, dist, keff, st);
    else if constexpr (FpsR<T>::v >= 16) fps_launch_resident<T, 16>(pts, c, rows, start, N, n, k, idx, dist, keff, st);
}

template <typename T>
void fps_stream(const void* pts, int c, const int32_t* rows, const int64_t* start, int N, int n, int k, int64_t* idx, void* dist, int32_t* keff, char* ws,
                const FpsLayout& L, hipStream_t st) {
    using T4 = typename V4<T>::type;
    const int G = fps_groups(n);
    const size_t total = (size_t)N * n;
    T4* rows4 = (T4*)(ws + L.rows4);
    FpsKey<T>* slots = (FpsKey<T>*)(ws + L.slots);
    fps_pack_kernel<T><<<(unsigned)((total + BLOCK - 1) / BLOCK), BLOCK, 0, st>>>((const T*)pts, c, rows, n, total, rows4, keff, N);
    for (int s = 0; s <= k; ++s)
        fps_stream_kernel<T><<<(unsigned)N * (unsigned)G, BLOCK, 0, st>>>(rows4, rows, start, N, n, G, s, k, slots, idx, (T*)dist, keff);
}

}  // namespace

void dicp_fps_geometry(int dtype, int* threads, int* resident_rows, int* stream_rows) {
    if (threads) *threads = FPS_THREADS;
    if (resident_rows) *resident_rows = bad_dtype(dtype) ? 0 : fps_resident_rows(dtype);
    if (stream_rows) *stream_rows = FPS_STREAM_ROWS;
}

size_t dicp_fps_workspace_bytes(int dtype, int N, int n, int k, int form) {
    if (fps_check(dtype, N, n, k, 3) || form < DICP_FPS_AUTO || form > DICP_FPS_STREAMED) return 0;
    return fps_streamed(dtype, n, form) ? fps_layout(dtype, N, n).total : 0;
}

int dicp_fps_forward(int dtype, const void* pts, int c, const int32_t* rows, const int64_t* start, int N, int n, int k, int form,
                     void* out, int64_t* idx, void* dist, int32_t* k_eff, void* workspace, size_t workspace_bytes, void* stream) {
    if (!pts || !out || !idx || !dist || !k_eff) return DICP_ERR_NULL;
    int rc = fps_check(dtype, N, n, k, c);
    if (rc) return rc;
    if (form < DICP_FPS_AUTO || form > DICP_FPS_STREAMED) return DICP_ERR_ENUM;
    if (form == DICP_FPS_RESIDENT && n > fps_resident_rows(dtype)) return DICP_ERR_SHAPE;
    if ((size_t)N * k >= ((size_t)1 << 40)) return DICP_ERR_SHAPE;
    const bool streamed = fps_streamed(dtype, n, form);
    const size_t ts = elem_size(dtype);
    const FpsLayout L = fps_layout(dtype, N, n);
    if (streamed) {
        if (!workspace) return DICP_ERR_NULL;
        if (workspace_bytes < L.total) return DICP_ERR_SHAPE;
        if (misaligned(workspace, 256)) return DICP_ERR_ALIGN;
    }
    if (misaligned(pts, ts) || misaligned(out, ts) || misaligned(dist, ts) || misaligned(idx, 8) || misaligned(k_eff, 4) || misaligned(rows, 4) || misaligned(start, 8))
        return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const size_t cells = (size_t)N * k * c;
    const unsigned gg = (unsigned)((cells + BLOCK - 1) / BLOCK);
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        if (streamed) fps_stream<T>(pts, c, rows, start, N, n, k, idx, dist, k_eff, (char*)workspace, L, st);
        else fps_resident<T>(pts, c, rows, start, N, n, k, idx, dist, k_eff, st);
        fps_gather_kernel<T><<<gg, BLOCK, 0, st>>>((const T*)pts, idx, n, k, c, cells, (T*)out);
    });
    return launch_status();
}

int dicp_fps_backward(int dtype, const void* grad_out, const int64_t* idx, int N, int n, int k, int c, void* grad_pts, void* stream) {
    if (!grad_out || !idx || !grad_pts) return DICP_ERR_NULL;
    int rc = fps_check(dtype, N, n, k, c);
    if (rc) return rc;
    const size_t ts = elem_size(dtype);
    if (misaligned(grad_out, ts) || misaligned(grad_pts, ts) || misaligned(idx, 8)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = dicp_fill::zero(grad_pts, (size_t)N * n * c * ts, st))) return rc;
    const size_t cells = (size_t)N * k * c;
    const unsigned gg = (unsigned)((cells + BLOCK - 1) / BLOCK);
    begin_launch();
    if (dtype == DICP_F32) fps_scatter_kernel<float><<<gg, BLOCK, 0, st>>>((const float*)grad_out, idx, n, k, c, cells, (float*)grad_pts);
    else                   fps_scatter_kernel<double><<<gg, BLOCK, 0, st>>>((const double*)grad_out, idx, n, k, c, cells, (double*)grad_pts);
    return launch_status();
}
