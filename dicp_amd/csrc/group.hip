// Neighbourhood features (dicp_amd/group.py): gather, interpolate and pool the rows of a feature table (N,m,C) through the (N,n,k) index
// tensors of ball_query / knn_points, with their backward passes.  The per-slot rules are csrc/dicp_group.h's.
//
// All of it is memory traffic, so the kernels differ only in how threads are laid over it.  Two forms, chosen on the host by the row size:
//   wide   (C * sizeof(T) >= 128 bytes): ONE WAVE PER QUERY.  Lanes 0..k-1 load the query's k indices once and turn them into row numbers
//          (-1: empty); the wave reads them by shuffles in wave-uniform loops.  Lanes then run along the channels, so a gathered row and an
//          output row are one contiguous segment each; 16-byte accesses where C * sizeof(T) and the bases are multiples of 16 (V > 1),
//          otherwise one element per lane (V = 1: C = 33, 65, 130, or a misaligned view).  group_points lays its lanes over the query's
//          whole (slot, channel) block, which is contiguous in the output.
//   narrow (C = 1, 3, 4, 6 ...): lanes over the flattened (query, slot, channel) / (query, channel) / (query, slot) space, so that stores
//          stay contiguous; a wave per query would leave most of its lanes idle.
// Backward into the features is a scatter-add with float atomics (unsafeAtomicAdd: one global_atomic_add per element, no compare-and-swap
// loop), one element per lane: a wave adds 256 contiguous bytes of one row at C = 64 float32.  group_points' backward is flat in both
// forms -- consecutive lanes are consecutive (slot, channel) elements, the same addresses a wave per query would add to.  g_centers and
// g_d2 are written once per element without atomics; g_d2's channel sum is per-lane partial sums in channel order, then a butterfly.
// pool_neighbors' wide forward does not give a query a whole wave: a query gets a GROUP of G lanes, G the smallest power of two that
// holds the row's packs (8 <= G <= WAVE), and a wave works on WAVE / G queries at once -- at C = 64 float32 (16 packs of 16 bytes) four
// queries per wave and every lane busy, where a wave per query keeps 16 of 64.  See pool_fwd_wide_kernel.
// Every kernel is a grid-stride loop of at most GROUP_MAX_BLOCKS workgroups with 64-bit element counts.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "dicp_common.h"
#include "dicp_fill.h"
#include "dicp_group.h"
#include "dicp_group_launch.h"

namespace {

constexpr int GW = BLOCK / WAVE;                    // waves (queries in flight) per workgroup of the wide form
constexpr size_t GROUP_WIDE_BYTES = 128;
static_assert(GROUP_K_MAX <= WAVE, "a query's slots fit the lanes of one wave");

// lane s < k: the row of slot s of query q (-1: empty); -1 in the other lanes
template <typename I>
__device__ __forceinline__ int lane_row(const I* __restrict__ idx, size_t q, int k, int lane, int nb) {
    return lane < k ? group_row(idx[q * k + lane], nb) : -1;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) x = x + __shfl_xor(x, off);
    return x;
}

// ------------------------------------------------------------------ group_points
template <typename T, typename I, int V>
__global__ __launch_bounds__(BLOCK) void group_fwd_wide_kernel(const T* __restrict__ f, const I* __restrict__ idx, const int32_t* __restrict__ rows,
                                                               const T* __restrict__ cen, int Cc, size_t Q, int n, int m, int k, int C, T* __restrict__ out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int VR = C / V, items = k * VR;
    for (size_t q = (size_t)blockIdx.x * GW + threadIdx.x / WAVE; q < Q; q += (size_t)gridDim.x * GW) {
        const size_t b = q / n;
        const int jr = lane_row(idx, q, k, lane, rows_of(rows, (int)b, m));
        const T* F = f + b * m * C;
        T* O = out + q * k * C;
        for (int i0 = 0; i0 < items; i0 += WAVE) {          // (wave-uniform trips: the shuffle needs every lane)
            const int item = i0 + lane;
            const bool on = item < items;
            const int s = on ? item / VR : 0;
            const int j = __shfl(jr, s);
            if (!on) continue;
            const int c = (item - s * VR) * V;
            Pack<T, V> x;
#pragma unroll
            for (int e = 0; e < V; ++e) x.v[e] = T(0);
            if (j >= 0) {
                x = pack_load<T, V>(F + (size_t)j * C + c);
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (c + e < Cc) x.v[e] = group_value<T>(x.v[e], cen[q * Cc + c + e], true);
            }
            pack_store<T, V>(O + (size_t)item * V, x);
        }
    }
}

template <typename T, typename I>
__global__ __launch_bounds__(BLOCK) void group_fwd_narrow_kernel(const T* __restrict__ f, const I* __restrict__ idx, const int32_t* __restrict__ rows,
                                                                 const T* __restrict__ cen, int Cc, size_t total, int n, int m, int k, int C, T* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLOCK) {
        const size_t slot = i / C;
        const int c = (int)(i - slot * C);
        const size_t q = slot / k, b = q / n;
        const int j = group_row(idx[slot], rows_of(rows, (int)b, m));
        T v = T(0);
        if (j >= 0) v = group_value<T>(f[(b * m + (size_t)j) * C + c], c < Cc ? cen[q * Cc + c] : T(0), c < Cc);
        out[i] = v;
    }
}

// g_features (zeroed) += g_out over the live slots: one element per lane, consecutive lanes consecutive (slot, channel) elements
template <typename T, typename I>
__global__ __launch_bounds__(BLOCK) void group_bwd_kernel(const T* __restrict__ g, const I* __restrict__ idx, const int32_t* __restrict__ rows,
                                                          size_t total, int n, int m, int k, int C, T* __restrict__ gf) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLOCK) {
        const size_t slot = i / C;
        const int c = (int)(i - slot * C);
        const size_t b = slot / k / n;
        const int j = group_row(idx[slot], rows_of(rows, (int)b, m));
        if (j >= 0) unsafeAtomicAdd(gf + (b * m + (size_t)j) * C + c, g[i]);
    }
}

// g_centers[q, c] = -(sum of g_out[q, s, c] over the live slots in slot order), 0 without a live slot: written once
template <typename T, typename I>
__global__ __launch_bounds__(BLOCK) void group_gcenters_kernel(const T* __restrict__ g, const I* __restrict__ idx, const int32_t* __restrict__ rows,
                                                               int Cc, size_t total, int n, int m, int k, int C, T* __restrict__ gc) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLOCK) {
        const size_t q = i / Cc;
        const int c = (int)(i - q * Cc);
        const int nb = rows_of(rows, (int)(q / n), m);
        T acc = T(0);
        int cnt = 0;
        for (int s = 0; s < k; ++s)
            if (group_row(idx[q * k + s], nb) >= 0) { acc = acc + g[(q * k + s) * C + c]; ++cnt; }
        gc[i] = cnt ? -acc : T(0);
    }
}

// ------------------------------------------------------------------ interpolate_features
// lane s < k: the slot's row (-1: empty index or non-finite d2) and r_s (0 for an empty slot); R in every lane, in slot order
template <typename T, typename I>
__device__ __forceinline__ void interp_lanes(const I* __restrict__ idx, const T* __restrict__ d2, T eps, size_t q, int k, int lane, int nb, int& jr, T& r, T& R) {
    jr = lane_row(idx, q, k, lane, nb);
    r = T(0);
    if (jr >= 0) {
        const T d = d2[q * k + lane];
        if (group_finite(d)) r = interp_r<T>(d, eps); else jr = -1;
    }
    R = T(0);
    for (int s = 0; s < k; ++s) R = R + __shfl(r, s);       // (an empty slot adds 0: exact)
}

// the same for one thread: R over the query's slots
template <typename T, typename I>
__device__ __forceinline__ int interp_slot(const I* __restrict__ idx, const T* __restrict__ d2, T eps, size_t o, int nb, T& r) {
    int j = group_row(idx[o], nb);
    r = T(0);
    if (j >= 0) {
        const T d = d2[o];
        if (group_finite(d)) r = interp_r<T>(d, eps); else j = -1;
    }
    return j;
}

template <typename T, typename I, int V>
__global__ __launch_bounds__(BLOCK) void interp_fwd_wide_kernel(const T* __restrict__ f, const I* __restrict__ idx, const int32_t* __restrict__ rows, const T* __restrict__ d2, T eps,
                                                                size_t Q, int n, int m, int k, int C, T* __restrict__ out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int VR = C / V;
    for (size_t q = (size_t)blockIdx.x * GW + threadIdx.x / WAVE; q < Q; q += (size_t)gridDim.x * GW) {
        const size_t b = q / n;
        int jr;
        T r, R;
        interp_lanes<T, I>(idx, d2, eps, q, k, lane, rows_of(rows, (int)b, m), jr, r, R);
        const T w = interp_w<T>(r, R);
        const T* F = f + b * m * C;
        for (int v0 = 0; v0 < VR; v0 += WAVE) {
            const bool on = v0 + lane < VR;
            const int c = (v0 + lane) * V;
            Pack<T, V> acc;
#pragma unroll
            for (int e = 0; e < V; ++e) acc.v[e] = T(0);
            for (int s = 0; s < k; ++s) {
                const int j = __shfl(jr, s);
                const T ws = __shfl(w, s);
                if (j < 0 || !on) continue;
                const Pack<T, V> x = pack_load<T, V>(F + (size_t)j * C + c);
#pragma unroll
                for (int e = 0; e < V; ++e) acc.v[e] = interp_add<T>(acc.v[e], ws, x.v[e]);
            }
            if (on) pack_store<T, V>(out + q * C + c, acc);
        }
    }
}

template <typename T, typename I>
__global__ __launch_bounds__(BLOCK) void interp_fwd_narrow_kernel(const T* __restrict__ f, const I* __restrict__ idx, const int32_t* __restrict__ rows, const T* __restrict__ d2, T eps,
                                                                  size_t total, int n, int m, int k, int C, T* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLOCK) {
        const size_t q = i / C;
        const int c = (int)(i - q * C);
        const size_t b = q / n;
        const int nb = rows_of(rows, (int)b, m);
        T R = T(0), r;
        for (int s = 0; s < k; ++s) {
            interp_slot<T, I>(idx, d2, eps, q * k + s, nb, r);
            R = R + r;
        }
        T acc = T(0);
        for (int s = 0; s < k; ++s) {
            const int j = interp_slot<T, I>(idx, d2, eps, q * k + s, nb, r);
            if (j >= 0) acc = interp_add<T>(acc, interp_w<T>(r, R), f[(b * m + (size_t)j) * C + c]);
        }
        out[i] = acc;
    }
}

// gf (zeroed, optional) += w_s g_out; gd2 (optional) written once per slot by lane 0 of the query's wave
template <typename T, typename I>
__global__ __launch_bounds__(BLOCK) void interp_bwd_wide_kernel(const T* __restrict__ g, const T* __restrict__ f, const T* __restrict__ out, const I* __restrict__ idx,
                                                                const int32_t* __restrict__ rows, const T* __restrict__ d2, T eps, size_t Q, int n, int m, int k, int C,
                                                                T* __restrict__ gf, T* __restrict__ gd2) {
    const int lane = threadIdx.x & (WAVE - 1);
    for (size_t q = (size_t)blockIdx.x * GW + threadIdx.x / WAVE; q < Q; q += (size_t)gridDim.x * GW) {
        const size_t b = q / n;
        int jr;
        T r, R;
        interp_lanes<T, I>(idx, d2, eps, q, k, lane, rows_of(rows, (int)b, m), jr, r, R);
        const T w = interp_w<T>(r, R);
        const T* F = f + b * m * C;
        const T* G = g + q * C;
        const T* O = out + q * C;
        for (int s = 0; s < k; ++s) {
            const int j = __shfl(jr, s);                    // (wave-uniform, and so is the branch below)
            const T ws = __shfl(w, s), rs = __shfl(r, s);
            if (j < 0) {
                if (gd2 && lane == 0) gd2[q * k + s] = T(0);
                continue;
            }
            T dot = T(0);
            for (int c = lane; c < C; c += WAVE) {
                const T gc = G[c];
                if (gd2) dot = interp_dot_add<T>(dot, gc, F[(size_t)j * C + c], O[c]);
                if (gf) unsafeAtomicAdd(gf + (b * m + (size_t)j) * C + c, ws * gc);
            }
            if (gd2) {
                dot = wave_sum(dot);
                if (lane == 0) gd2[q * k + s] = interp_gd2<T>(rs, R, dot);
            }
        }
    }
}

// one thread per (query, slot)
template <typename T, typename I>
__global__ __launch_bounds__(BLOCK) void interp_bwd_narrow_kernel(const T* __restrict__ g, const T* __restrict__ f, const T* __restrict__ out, const I* __restrict__ idx,
                                                                  const int32_t* __restrict__ rows, const T* __restrict__ d2, T eps, size_t total, int n, int m, int k, int C,
                                                                  T* __restrict__ gf, T* __restrict__ gd2) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLOCK) {
        const size_t q = i / k;
        const size_t b = q / n;
        const int nb = rows_of(rows, (int)b, m);
        T R = T(0), r;
        for (int s = 0; s < k; ++s) {
            interp_slot<T, I>(idx, d2, eps, q * k + s, nb, r);
            R = R + r;
        }
        const int j = interp_slot<T, I>(idx, d2, eps, i, nb, r);
        if (j < 0) {
            if (gd2) gd2[i] = T(0);
            continue;
        }
        const T w = interp_w<T>(r, R);
        const T* Fj = f + (b * m + (size_t)j) * C;
        T dot = T(0);
        for (int c = 0; c < C; ++c) {
            const T gc = g[q * C + c];
            if (gd2) dot = interp_dot_add<T>(dot, gc, Fj[c], out[q * C + c]);
            if (gf) unsafeAtomicAdd(gf + (b * m + (size_t)j) * C + c, w * gc);
        }
        if (gd2) gd2[i] = interp_gd2<T>(r, R, dot);
    }
}

// ------------------------------------------------------------------ pool_neighbors
constexpr int POOL_U = 4;                           // row loads a lane keeps in flight (slots per unrolled step); every G is a multiple of it

// smallest power of two >= min(packs, WAVE), at least 8 (a wide row has at least 8 packs)
inline int pool_lanes(int packs) {
    int g = 8;
    while (g < packs && g < WAVE) g <<= 1;
    return g;
}

// G lanes per query, WAVE / G queries per wave, GW * WAVE / G per workgroup.  Lane gl of a group holds the row of slot s0 + gl; the group
// reads the rows by shuffles of width G, POOL_U slots a step: their row loads are issued together, then folded in slot order.  Every loop
// has wave-uniform trips and no lane leaves early (a query past Q holds -1 everywhere), so every shuffle's source lane is live.  A row of
// more than G packs (only at G = WAVE) loops over v0; its k <= 32 indices are then one s0 step.  MAX: best / its row per channel of
// the lane's pack, argmax stored as packs of V int32; otherwise the running sum, divided once by the count for the mean.
template <typename T, typename I, int V, bool MAX>
__global__ __launch_bounds__(BLOCK) void pool_fwd_wide_kernel(const T* __restrict__ f, const I* __restrict__ idx, const int32_t* __restrict__ rows, size_t Q, int n, int m, int k, int C,
                                                              int G, int mean, T* __restrict__ out, int32_t* __restrict__ amax, int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int gl = lane & (G - 1);
    const int QW = WAVE / G, VR = C / V;
    const size_t per_block = (size_t)GW * QW;
    const size_t q_in = (size_t)(threadIdx.x / WAVE) * QW + lane / G;
    for (size_t q0 = (size_t)blockIdx.x * per_block; q0 < Q; q0 += (size_t)gridDim.x * per_block) {
        const size_t q = q0 + q_in;
        const bool valid = q < Q;
        const size_t b = valid ? q / n : 0;
        const int nb = valid ? rows_of(rows, (int)b, m) : 0;
        const T* F = f + b * m * C;
        for (int v0 = 0; v0 < VR; v0 += G) {
            const bool on = valid && v0 + gl < VR;
            const int c = (v0 + gl) * V;
            Pack<T, V> acc;
            Pack<int32_t, V> arg;
#pragma unroll
            for (int e = 0; e < V; ++e) { acc.v[e] = T(0); arg.v[e] = -1; }
            int cnt = 0;
            for (int s0 = 0; s0 < k; s0 += G) {
                const int jr = (valid && s0 + gl < k) ? group_row(idx[q * k + s0 + gl], nb) : -1;
                const int lim = min(G, k - s0);
                for (int t0 = 0; t0 < lim; t0 += POOL_U) {
                    int j[POOL_U];
                    Pack<T, V> x[POOL_U];
#pragma unroll
                    for (int u = 0; u < POOL_U; ++u) j[u] = __shfl(jr, t0 + u, G);     // (a lane past lim holds -1)
#pragma unroll
                    for (int u = 0; u < POOL_U; ++u) {
#pragma unroll
                        for (int e = 0; e < V; ++e) x[u].v[e] = T(0);
                        if (on && j[u] >= 0) x[u] = pack_load<T, V>(F + (size_t)j[u] * C + c);
                    }
#pragma unroll
                    for (int u = 0; u < POOL_U; ++u) {
                        if (j[u] < 0) continue;
                        ++cnt;
#pragma unroll
                        for (int e = 0; e < V; ++e) {
                            if (MAX) pool_max_step<T>(x[u].v[e], j[u], acc.v[e], arg.v[e]);
                            else acc.v[e] = pool_sum_step<T>(acc.v[e], x[u].v[e]);
                        }
                    }
                }
            }
            if (on) {
                if (!MAX && mean) {
#pragma unroll
                    for (int e = 0; e < V; ++e) acc.v[e] = pool_mean<T>(acc.v[e], cnt);
                }
                pack_store<T, V>(out + q * C + c, acc);
                if (MAX) pack_store<int32_t, V>(amax + q * C + c, arg);
            }
            if (valid && v0 == 0 && gl == 0) counts[q] = cnt;
        }
    }
}

// one thread per (query, channel): out and argmax are stored contiguously along the flattened index.  The threads of a query (and, at
// C = 1, the 64 lanes of a wave) would read the query's k indices at a pitch of k elements, 64 cache lines an instruction; instead the
// workgroup turns the indices of its queries -- one contiguous range -- into row numbers (-1: empty) in LDS with coalesced loads, each
// index read once, at an odd pitch so that lanes of different queries are on different banks.  The slot loop is unrolled by POOL_U like
// the wide form's: the gathers of a step are issued before the first is folded.
template <typename T, typename I, bool MAX>
__global__ __launch_bounds__(BLOCK) void pool_fwd_narrow_kernel(const T* __restrict__ f, const I* __restrict__ idx, const int32_t* __restrict__ rows, size_t total, int n, int m, int k, int C,
                                                                int mean, T* __restrict__ out, int32_t* __restrict__ amax, int32_t* __restrict__ counts) {
    extern __shared__ int pool_rows[];                      // [(BLOCK - 1) / C + 2 queries][k | 1]
    const int pitch = k | 1;
    for (size_t i0 = (size_t)blockIdx.x * BLOCK; i0 < total; i0 += (size_t)gridDim.x * BLOCK) {        // (workgroup-uniform: the barriers)
        const size_t q_lo = i0 / C;
        const size_t last = (i0 + BLOCK < total ? i0 + BLOCK : total) - 1;
        const int nq = (int)(last / C - q_lo) + 1;          // <= (BLOCK - 1) / C + 2
        for (int t = threadIdx.x; t < nq * k; t += BLOCK) {
            const int ql = t / k, s = t - ql * k;
            const size_t q = q_lo + ql;
            pool_rows[ql * pitch + s] = group_row(idx[q * k + s], rows_of(rows, (int)(q / n), m));
        }
        __syncthreads();
        const size_t i = i0 + threadIdx.x;
        if (i < total) {
            const size_t q = i / C;
            const int c = (int)(i - q * C);
            const size_t b = q / n;
            const int* jr = pool_rows + (int)(q - q_lo) * pitch;
            const T* F = f + b * m * C + c;
            T acc = T(0);
            int arg = -1, cnt = 0;
            for (int s0 = 0; s0 < k; s0 += POOL_U) {
                int j[POOL_U];
                T x[POOL_U];
#pragma unroll
                for (int u = 0; u < POOL_U; ++u) j[u] = s0 + u < k ? jr[s0 + u] : -1;
#pragma unroll
                for (int u = 0; u < POOL_U; ++u) {
                    x[u] = T(0);
                    if (j[u] >= 0) x[u] = F[(size_t)j[u] * C];
                }
#pragma unroll
                for (int u = 0; u < POOL_U; ++u) {
                    if (j[u] < 0) continue;
                    ++cnt;
                    if (MAX) pool_max_step<T>(x[u], j[u], acc, arg);
                    else acc = pool_sum_step<T>(acc, x[u]);
                }
            }
            if (!MAX && mean) acc = pool_mean<T>(acc, cnt);
            out[i] = acc;
            if (MAX) amax[i] = arg;
            if (c == 0) counts[q] = cnt;
        }
        __syncthreads();                                    // (the next range overwrites the rows)
    }
}

// g_features (zeroed) [argmax[q, c], c] += g[q, c]: flat over (query, channel); -1 (no live slot) adds nothing.  The row goes through
// group_row again, so that nothing is added out of range whatever the argmax buffer holds
template <typename T>
__global__ __launch_bounds__(BLOCK) void pool_bwd_max_kernel(const T* __restrict__ g, const int32_t* __restrict__ amax, const int32_t* __restrict__ rows, size_t total, int n, int m, int C,
                                                             T* __restrict__ gf) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLOCK) {
        const size_t q = i / C;
        const int c = (int)(i - q * C);
        const size_t b = q / n;
        const int j = group_row(amax[i], rows_of(rows, (int)b, m));
        if (j >= 0) unsafeAtomicAdd(gf + (b * m + (size_t)j) * C + c, g[i]);
    }
}

// g_features (zeroed) += g[q, :] (divided by the count: counts != NULL, the mean) over the live slots: flat over (query, slot, channel) as
// group_bwd_kernel, the cotangent read per query instead of per slot
template <typename T, typename I>
__global__ __launch_bounds__(BLOCK) void pool_bwd_sum_kernel(const T* __restrict__ g, const I* __restrict__ idx, const int32_t* __restrict__ rows, const int32_t* __restrict__ counts,
                                                             size_t total, int n, int m, int k, int C, T* __restrict__ gf) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLOCK) {
        const size_t slot = i / C;
        const int c = (int)(i - slot * C);
        const size_t q = slot / k, b = q / n;
        const int j = group_row(idx[slot], rows_of(rows, (int)b, m));
        if (j < 0) continue;
        T v = g[q * C + c];
        if (counts) v = pool_mean_grad<T>(v, counts[q]);
        unsafeAtomicAdd(gf + (b * m + (size_t)j) * C + c, v);
    }
}

// ------------------------------------------------------------------ host side
inline bool wide(int dtype, int C) { return (size_t)C * elem_size(dtype) >= GROUP_WIDE_BYTES; }

}  // namespace

int dicp_group_forward(int dtype, const void* features, const void* idx, int idx64, const int32_t* rows, const void* centers, int Cc,
                       int N, int n, int m, int k, int C, void* out, void* stream) {
    if (!features || !idx || !out || (Cc != 0 && !centers)) return DICP_ERR_NULL;
    int rc = group_check(dtype, idx64, N, n, m, k, C);
    if (rc) return rc;
    if (Cc < 0 || Cc > C) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(features, ts) || misaligned(out, ts) || misaligned(centers, ts) || misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const size_t Q = (size_t)N * n, total = Q * k * C;
    const bool w = wide(dtype, C), v = w && vec16(dtype, C, features, out);
    begin_launch();
    with_scalar_index(dtype, idx64, [&](auto t, auto i) {
        using T = decltype(t);
        using I = decltype(i);
        if (v)      group_fwd_wide_kernel<T, I, VecOf<T>::v><<<group_grid(Q, GW), BLOCK, 0, st>>>((const T*)features, (const I*)idx, rows, (const T*)centers, Cc, Q, n, m, k, C, (T*)out);
        else if (w) group_fwd_wide_kernel<T, I, 1><<<group_grid(Q, GW), BLOCK, 0, st>>>((const T*)features, (const I*)idx, rows, (const T*)centers, Cc, Q, n, m, k, C, (T*)out);
        else        group_fwd_narrow_kernel<T, I><<<group_grid(total, BLOCK), BLOCK, 0, st>>>((const T*)features, (const I*)idx, rows, (const T*)centers, Cc, total, n, m, k, C, (T*)out);
    });
    return launch_status();
}

int dicp_group_backward(int dtype, const void* grad_out, const void* idx, int idx64, const int32_t* rows, int Cc,
                        int N, int n, int m, int k, int C, void* grad_features, void* grad_centers, void* stream) {
    if (!grad_out || !idx || (!grad_features && !grad_centers)) return DICP_ERR_NULL;
    int rc = group_check(dtype, idx64, N, n, m, k, C);
    if (rc) return rc;
    if (Cc < 0 || Cc > C || (grad_centers && Cc == 0)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(grad_out, ts) || misaligned(grad_features, ts) || misaligned(grad_centers, ts) || misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const size_t Q = (size_t)N * n, total = Q * k * C, ctotal = Q * Cc;
    if (grad_features && (rc = dicp_fill::zero(grad_features, (size_t)N * m * C * ts, st))) return rc;
    begin_launch();
    with_scalar_index(dtype, idx64, [&](auto t, auto i) {
        using T = decltype(t);
        using I = decltype(i);
        if (grad_features) group_bwd_kernel<T, I><<<group_grid(total, BLOCK), BLOCK, 0, st>>>((const T*)grad_out, (const I*)idx, rows, total, n, m, k, C, (T*)grad_features);
        if (grad_centers)  group_gcenters_kernel<T, I><<<group_grid(ctotal, BLOCK), BLOCK, 0, st>>>((const T*)grad_out, (const I*)idx, rows, Cc, ctotal, n, m, k, C, (T*)grad_centers);
    });
    return launch_status();
}

int dicp_interpolate_forward(int dtype, const void* features, const void* idx, int idx64, const int32_t* rows, const void* d2, double eps,
                             int N, int n, int m, int k, int C, void* out, void* stream) {
    if (!features || !idx || !d2 || !out) return DICP_ERR_NULL;
    int rc = group_check(dtype, idx64, N, n, m, k, C);
    if (rc) return rc;
    if (!(eps > 0.0) || eps - eps != 0.0) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(features, ts) || misaligned(out, ts) || misaligned(d2, ts) || misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const size_t Q = (size_t)N * n, total = Q * C;
    const bool w = wide(dtype, C), v = w && vec16(dtype, C, features, out);
    begin_launch();
    with_scalar_index(dtype, idx64, [&](auto t, auto i) {
        using T = decltype(t);
        using I = decltype(i);
        if (v)      interp_fwd_wide_kernel<T, I, VecOf<T>::v><<<group_grid(Q, GW), BLOCK, 0, st>>>((const T*)features, (const I*)idx, rows, (const T*)d2, (T)eps, Q, n, m, k, C, (T*)out);
        else if (w) interp_fwd_wide_kernel<T, I, 1><<<group_grid(Q, GW), BLOCK, 0, st>>>((const T*)features, (const I*)idx, rows, (const T*)d2, (T)eps, Q, n, m, k, C, (T*)out);
        else        interp_fwd_narrow_kernel<T, I><<<group_grid(total, BLOCK), BLOCK, 0, st>>>((const T*)features, (const I*)idx, rows, (const T*)d2, (T)eps, total, n, m, k, C, (T*)out);
    });
    return launch_status();
}

int dicp_interpolate_backward(int dtype, const void* grad_out, const void* features, const void* out, const void* idx, int idx64, const int32_t* rows,
                              const void* d2, double eps, int N, int n, int m, int k, int C, void* grad_features, void* grad_d2, void* stream) {
    if (!grad_out || !features || !out || !idx || !d2 || (!grad_features && !grad_d2)) return DICP_ERR_NULL;
    int rc = group_check(dtype, idx64, N, n, m, k, C);
    if (rc) return rc;
    if (!(eps > 0.0) || eps - eps != 0.0) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(grad_out, ts) || misaligned(features, ts) || misaligned(out, ts) || misaligned(d2, ts) || misaligned(grad_features, ts) || misaligned(grad_d2, ts)
        || misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const size_t Q = (size_t)N * n, total = Q * k;
    if (grad_features && (rc = dicp_fill::zero(grad_features, (size_t)N * m * C * ts, st))) return rc;
    const bool w = wide(dtype, C);
    begin_launch();
    with_scalar_index(dtype, idx64, [&](auto t, auto i) {
        using T = decltype(t);
        using I = decltype(i);
        if (w) interp_bwd_wide_kernel<T, I><<<group_grid(Q, GW), BLOCK, 0, st>>>((const T*)grad_out, (const T*)features, (const T*)out, (const I*)idx, rows, (const T*)d2, (T)eps,
                                                                                 Q, n, m, k, C, (T*)grad_features, (T*)grad_d2);
        else   interp_bwd_narrow_kernel<T, I><<<group_grid(total, BLOCK), BLOCK, 0, st>>>((const T*)grad_out, (const T*)features, (const T*)out, (const I*)idx, rows, (const T*)d2, (T)eps,
                                                                                        total, n, m, k, C, (T*)grad_features, (T*)grad_d2);
    });
    return launch_status();
}

int dicp_pool_forward(int dtype, const void* features, const void* idx, int idx64, const int32_t* rows, int reduce,
                      int N, int n, int m, int k, int C, void* out, int32_t* argmax, int32_t* counts, void* stream) {
    if (!features || !idx || !out || !counts) return DICP_ERR_NULL;
    if (reduce != DICP_POOL_SUM && reduce != DICP_POOL_MEAN && reduce != DICP_POOL_MAX) return DICP_ERR_ENUM;
    if (reduce == DICP_POOL_MAX && !argmax) return DICP_ERR_NULL;
    if (reduce != DICP_POOL_MAX && argmax) return DICP_ERR_ENUM;
    int rc = group_check(dtype, idx64, N, n, m, k, C);
    if (rc) return rc;
    const size_t ts = elem_size(dtype);
    if (misaligned(features, ts) || misaligned(out, ts) || misaligned(argmax, 4) || misaligned(counts, 4) || misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const size_t Q = (size_t)N * n, total = Q * C;
    const bool w = wide(dtype, C), v = w && vec16(dtype, C, features, out) && !((uintptr_t)argmax & 15);
    const int G = pool_lanes(v ? C / (int)(16 / ts) : C), per_block = GW * (WAVE / G), mean = reduce == DICP_POOL_MEAN;
    const size_t narrow_lds = (size_t)((BLOCK - 1) / C + 2) * (k | 1) * sizeof(int);     // at most 257 x 33 x 4 bytes
    begin_launch();
    with_scalar_index(dtype, idx64, [&](auto t, auto i) {
        using T = decltype(t);
        using I = decltype(i);
        auto launch = [&](auto is_max) {
            constexpr bool MAX = decltype(is_max)::value;
            if (v)      pool_fwd_wide_kernel<T, I, VecOf<T>::v, MAX><<<group_grid(Q, per_block), BLOCK, 0, st>>>((const T*)features, (const I*)idx, rows, Q, n, m, k, C, G, mean, (T*)out, argmax, counts);
            else if (w) pool_fwd_wide_kernel<T, I, 1, MAX><<<group_grid(Q, per_block), BLOCK, 0, st>>>((const T*)features, (const I*)idx, rows, Q, n, m, k, C, G, mean, (T*)out, argmax, counts);
            else        pool_fwd_narrow_kernel<T, I, MAX><<<group_grid(total, BLOCK), BLOCK, narrow_lds, st>>>((const T*)features, (const I*)idx, rows, total, n, m, k, C, mean, (T*)out, argmax, counts);
        };
        if (reduce == DICP_POOL_MAX) launch(std::true_type());
        else launch(std::false_type());
    });
    return launch_status();
}

int dicp_pool_backward(int dtype, const void* grad_out, const void* idx, int idx64, const int32_t* rows, int reduce,
                       const int32_t* argmax, const int32_t* counts, int N, int n, int m, int k, int C, void* grad_features, void* stream) {
    if (!grad_out || !idx || !grad_features) return DICP_ERR_NULL;
    if (reduce != DICP_POOL_SUM && reduce != DICP_POOL_MEAN && reduce != DICP_POOL_MAX) return DICP_ERR_ENUM;
    if ((reduce == DICP_POOL_MAX && !argmax) || (reduce == DICP_POOL_MEAN && !counts)) return DICP_ERR_NULL;
    if (reduce != DICP_POOL_MAX && argmax) return DICP_ERR_ENUM;
    int rc = group_check(dtype, idx64, N, n, m, k, C);
    if (rc) return rc;
    const size_t ts = elem_size(dtype);
    if (misaligned(grad_out, ts) || misaligned(grad_features, ts) || misaligned(argmax, 4) || misaligned(counts, 4) || misaligned(idx, idx64 ? 8 : 4) || misaligned(rows, 4)) return DICP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const size_t Q = (size_t)N * n, qc = Q * C, total = qc * k;
    if ((rc = dicp_fill::zero(grad_features, (size_t)N * m * C * ts, st))) return rc;
    const int32_t* cnt = reduce == DICP_POOL_MEAN ? counts : nullptr;
    begin_launch();
    if (reduce == DICP_POOL_MAX) {
        if (dtype == DICP_F32) pool_bwd_max_kernel<float><<<group_grid(qc, BLOCK), BLOCK, 0, st>>>((const float*)grad_out, argmax, rows, qc, n, m, C, (float*)grad_features);
        else                   pool_bwd_max_kernel<double><<<group_grid(qc, BLOCK), BLOCK, 0, st>>>((const double*)grad_out, argmax, rows, qc, n, m, C, (double*)grad_features);
    } else {
        with_scalar_index(dtype, idx64, [&](auto t, auto i) {
            using T = decltype(t);
            using I = decltype(i);
            pool_bwd_sum_kernel<T, I><<<group_grid(total, BLOCK), BLOCK, 0, st>>>((const T*)grad_out, (const I*)idx, rows, cnt, total, n, m, k, C, (T*)grad_features);
        });
    }
    return launch_status();
}
