// Whole-ball FPFH descriptors for batches of clouds, at every row or at chosen rows (dicp_amd/fpfh.py: fpfh_features_ball /
// compute_fpfh(whole_ball=True)).  The rules are csrc/dicp_fpfh.h's, the near list and its order csrc/dicp_fpfh_ball.h's, the walk and its
// coverage proof csrc/dicp_iss_ball.h's; the grid is the one dicp_ball_grid_build makes (csrc/ball_query.hip), read here and never built.
// No index and no d2 tensor is written or read.  Everything is in double with no float atomics and nothing read back: every pass is
// bit-reproducible and equals tests/fpfh_ball_ref.py bit for bit.
//
// The workspace (dicp_fpfh_ball_workspace_bytes) holds, 256-byte aligned and in this order:
//   table  (N, m, FPFH_BALL_ROW) double: per SORTED SLOT s < cnt the 33 values s_j[ch] = fpfh_spfh(cnt, c) and the OK flag -- formed once
//          per row by pass 1 instead of once per (row, member) by pass 2: no division is left in pass 2's walk;
//   nrm4   (N, m, 4) T: per sorted slot the row's normal and its OK flag (1 / 0), so that pass 1 never gathers through perm;
//   inv    (N, m) int32: the sorted slot of every row, -1 for a row outside the grid.
// Pack (dicp_fpfh_ball_pack), one lane per sorted slot: nrm4 for the slots below the plan's count; inv for every perm[s] < m -- the sort
//   leaves every index once, so every row's inv is stored once.
// Pass 1 (dicp_fpfh_ball_spfh), one lane per sorted slot, one wave per workgroup (the lanes of a wave are 64 consecutive rows of the cell
//   order and walk the same cells): a lane walks its ball once and adds 1 to three of its 33 counters per pair.  The counters are
//   lane-private LDS columns cnt[channel][lane] (8448 bytes a wave; 33 dynamically indexed registers would go to scratch): whatever
//   channel a lane picks, its word lies in bank lane % 32 -- no conflicts, no cross-lane sharing, plain integer adds.
//   The epilogue writes the slot's table row and, where asked for, the int32 counts of the ORIGINAL row perm[s]; a lane whose perm is
//   below m stores its row's counts (zeros for a row outside the grid), the padding lanes store nothing: every element once.
// Pass 2 (dicp_fpfh_ball_combine), one walk with the 33 sums in registers, two launch forms of one kernel:
//   at == NULL: a lane per sorted slot, the 33 results scattered to row perm[s] of out (N, m, 33);
//   at != NULL: a lane per entry of at (N, q): its slot through inv, its point rows4[slot] (the row's own coordinates, bit for bit), the
//     results to entry e of out (N, q, 33) -- 300 keypoints of 16384 rows cost 300 walks, not 16384 lanes of which most idle.
//   Per near row one gathered table row (272 bytes), 33 products and 33 additions; the row's own table row is read after the walk.
// `visited` (optional, for scripts/fpfh_ball_bench.py): the rows visited per cloud, added to the caller's zeroed counters with integer
//   atomics, one per lane -- a diagnostic that slows the pass down and touches no output.
// No spin-waits, no cooperative launch; every loop is bounded by the cloud's row count (iss_ball_scan's bound); the plan's count is
// clamped to m before any load, and every slot read from inv is clamped to the count.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_fpfh_ball.h"
#include "kernels_grid_plan.h"

namespace {

template <typename T>
__device__ __forceinline__ BallPlan<T> clamped_plan(const void* plans, int b, int m) {
    BallPlan<T> pl = plan_of<T>(plans, b);
    pl.cnt = min(max(pl.cnt, 0), m);                                    // (the grid's own count: the clamp is a belt for the loads below)
    return pl;
}

// ------------------------------------------------------------------ pack
template <typename T>
__global__ __launch_bounds__(BLOCK) void fpfh_ball_pack_kernel(const void* __restrict__ plans, const int32_t* __restrict__ perm,
                                                               const typename V4<T>::type* __restrict__ rows4, const T* __restrict__ nrm, int m,
                                                               int Pm, int bpc, typename V4<T>::type* __restrict__ nrm4, int32_t* __restrict__ inv) {
    using T4 = typename V4<T>::type;
    const int b = blockIdx.x / bpc, s = (blockIdx.x - b * bpc) * BLOCK + threadIdx.x;
    if (s >= Pm) return;
    const size_t gbase = (size_t)b * Pm, base = (size_t)b * m;
    const int i = perm[gbase + s];
    if (i < 0 || i >= m) return;                                        // the padding of the sort: no row
    const int cnt = min(max(plan_of<T>(plans, b).cnt, 0), m);
    const bool live = s < cnt;                                          // the live rows are the first cnt sorted slots
    if (live) {
        const T4 p = rows4[gbase + s];
        const T* n = nrm + (base + i) * 3;
        const T nx = n[0], ny = n[1], nz = n[2];
        const double pd[3] = {(double)p.x, (double)p.y, (double)p.z}, nd[3] = {(double)nx, (double)ny, (double)nz};
        T4 o;
        o.x = nx; o.y = ny; o.z = nz; o.w = fpfh_row_ok(pd, nd) ? T(1) : T(0);
        nrm4[base + s] = o;                                             // (s < cnt <= m)
    }
    inv[base + i] = live ? s : -1;
}

// ------------------------------------------------------------------ pass 1
template <typename T>
__global__ __launch_bounds__(WAVE) void fpfh_ball_spfh_kernel(const void* __restrict__ plans, const uint64_t* __restrict__ keys,
                                                              const int32_t* __restrict__ perm, const typename V4<T>::type* __restrict__ rows4,
                                                              const typename V4<T>::type* __restrict__ nrm4, int m, int Pm, int bpc, double radius,
                                                              double* __restrict__ table, int32_t* __restrict__ spfh,
                                                              unsigned long long* __restrict__ visited_out) {
    using T4 = typename V4<T>::type;
    __shared__ int cnt[FPFH_CH * WAVE];                                 // [channel][lane]: a lane's 33 counters, a column of its own
    const int lane = threadIdx.x;
    const int b = blockIdx.x / bpc, s = (blockIdx.x - b * bpc) * WAVE + lane;
    if (s >= Pm) return;
    const size_t gbase = (size_t)b * Pm, base = (size_t)b * m;
    const int i = perm[gbase + s];
    if (i < 0 || i >= m) return;                                        // the padding of the sort: no row of the outputs
    const BallPlan<T> pl = clamped_plan<T>(plans, b, m);
#pragma unroll
    for (int ch = 0; ch < FPFH_CH; ++ch) cnt[ch * WAVE + lane] = 0;
    const bool live = s < pl.cnt;
    if (live) {
        const T4 n4 = nrm4[base + s];
        const bool ok = n4.w != T(0);
        if (ok) {
            const uint64_t* kb = keys + gbase;
            const T4* nb = nrm4 + base;
            const double ni[3] = {(double)n4.x, (double)n4.y, (double)n4.z};
            auto key = [&](int j) -> uint64_t { return kb[j]; };
            auto row = [&](int j) -> T4 { return rows4[gbase + j]; };
            auto nrm = [&](int j, double* n) -> bool {
                const T4 v = nb[j];
                n[0] = (double)v.x; n[1] = (double)v.y; n[2] = (double)v.z;
                return v.w != T(0);
            };
            auto add = [&](const int* ch) {
                cnt[ch[0] * WAVE + lane] += 1;
                cnt[ch[1] * WAVE + lane] += 1;
                cnt[ch[2] * WAVE + lane] += 1;
            };
            const unsigned visited = fpfh_ball_spfh_row<T>(pl, iss_ball_R<T>(radius), radius * radius, s, ni, key, row, nrm, add);
            if (visited_out) atomicAdd(visited_out + b, (unsigned long long)visited);        // diagnostics only: an integer count
        }
        fpfh_ball_table_row([&](int ch) -> int { return cnt[ch * WAVE + lane]; }, ok, table + (base + s) * FPFH_BALL_ROW);
    }
    if (spfh) {
        int32_t* o = spfh + (base + i) * FPFH_CH;
#pragma unroll
        for (int ch = 0; ch < FPFH_CH; ++ch) o[ch] = cnt[ch * WAVE + lane];
    }
}

// ------------------------------------------------------------------ pass 2
template <typename T, typename I>
__global__ __launch_bounds__(WAVE) void fpfh_ball_combine_kernel(const void* __restrict__ plans, const uint64_t* __restrict__ keys,
                                                                 const int32_t* __restrict__ perm, const typename V4<T>::type* __restrict__ rows4,
                                                                 const I* __restrict__ at, int q, int m, int Pm, int bpc, double radius,
                                                                 const double* __restrict__ table, const int32_t* __restrict__ inv,
                                                                 T* __restrict__ out, unsigned long long* __restrict__ visited_out) {
    using T4 = typename V4<T>::type;
    const int b = blockIdx.x / bpc, e = (blockIdx.x - b * bpc) * WAVE + threadIdx.x;
    const size_t gbase = (size_t)b * Pm, base = (size_t)b * m;
    const BallPlan<T> pl = clamped_plan<T>(plans, b, m);
    int s;
    size_t o;                                                           // the row of `out` this lane stores
    if (at) {
        if (e >= q) return;
        const int32_t* ib = inv + base;
        s = fpfh_ball_at(at[(size_t)b * q + e], m, [&](int i) -> int { return ib[i]; });       // (pack wrote inv for every row i < m)
        o = (size_t)b * q + e;
    } else {
        if (e >= Pm) return;
        const int i = perm[gbase + e];
        if (i < 0 || i >= m) return;                                    // the padding of the sort: no row of out
        s = e;
        o = base + i;
    }
    if (s >= pl.cnt) s = -1;                                            // a row outside the grid (and the belt for the loads below)
    const double* tb = table + base * FPFH_BALL_ROW;
    double acc[FPFH_CH];
    bool ok = false;
    if (s >= 0) ok = tb[(size_t)s * FPFH_BALL_ROW + FPFH_CH] != 0.0;     // (pass 1 wrote the table row of every slot below cnt)
    T* dst = out + o * FPFH_CH;
    if (!ok) {
#pragma unroll
        for (int ch = 0; ch < FPFH_CH; ++ch) dst[ch] = T(0);
        return;
    }
    const uint64_t* kb = keys + gbase;
    auto key = [&](int j) -> uint64_t { return kb[j]; };
    auto row = [&](int j) -> T4 { return rows4[gbase + j]; };
    auto tab = [&](int j) -> const double* { return tb + (size_t)j * FPFH_BALL_ROW; };
    const unsigned visited = fpfh_ball_combine_row<T>(pl, iss_ball_R<T>(radius), radius * radius, s, key, row, tab, acc);
    if (visited_out) atomicAdd(visited_out + b, (unsigned long long)visited);
    fpfh_ball_out(acc, tab(s), [&](int ch, double v) { dst[ch] = (T)v; });
}

// ------------------------------------------------------------------ checks
inline size_t table_bytes(int N, int m) { return up256((size_t)N * m * FPFH_BALL_ROW * sizeof(double)); }
inline size_t nrm4_bytes(int dtype, int N, int m) { return up256((size_t)N * m * 4 * elem_size(dtype)); }
inline size_t inv_bytes(int N, int m) { return up256((size_t)N * m * sizeof(int32_t)); }
inline size_t workspace_bytes_of(int dtype, int N, int m) { return table_bytes(N, m) + nrm4_bytes(dtype, N, m) + inv_bytes(N, m); }

int fpfh_ball_shape(int dtype, int N, int m) {
    int rc = ball_check(dtype, N, m);
    if (rc) return rc;
    if ((size_t)N * (size_t)m >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;
    if ((size_t)N * (size_t)((ball_slots(m) + WAVE - 1) / WAVE) >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;
    return 0;
}
// the checks of the three entry points after the null checks, in the order that decides the status of a bad call
int fpfh_ball_check(int dtype, int N, int m, double radius, size_t workspace_bytes) {
    int rc = fpfh_ball_shape(dtype, N, m);
    if (rc) return rc;
    if (!(radius > 0.0 && radius < HUGE_VAL && radius * radius < HUGE_VAL)) return DICP_ERR_SHAPE;
    if (workspace_bytes < workspace_bytes_of(dtype, N, m)) return DICP_ERR_SHAPE;
    return 0;
}

struct Workspace {
    double* table;
    void* nrm4;
    int32_t* inv;
};
inline Workspace carve(const void* ws, int dtype, int N, int m) {
    char* p = (char*)ws;
    Workspace w;
    w.table = (double*)p;
    w.nrm4 = p + table_bytes(N, m);
    w.inv = (int32_t*)(p + table_bytes(N, m) + nrm4_bytes(dtype, N, m));
    return w;
}

}  // namespace

size_t dicp_fpfh_ball_workspace_bytes(int dtype, int N, int m) {
    if (fpfh_ball_shape(dtype, N, m)) return 0;
    return workspace_bytes_of(dtype, N, m);
}

int dicp_fpfh_ball_pack(int dtype, const void* plans, const int32_t* perm, const void* rows4, const void* normals, int N, int m, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (!plans || !perm || !rows4 || !normals || !workspace) return DICP_ERR_NULL;
    int rc = fpfh_ball_check(dtype, N, m, 1.0, workspace_bytes);
    if (rc) return rc;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(plans, 8) || misaligned(perm, 4) || misaligned(rows4, 4 * ts) || misaligned(normals, ts))
        return DICP_ERR_ALIGN;
    const int Pm = ball_slots(m), bpc = (Pm + BLOCK - 1) / BLOCK;
    const unsigned g = (unsigned)N * (unsigned)bpc;
    const Workspace w = carve(workspace, dtype, N, m);
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        using T4 = typename V4<T>::type;
        fpfh_ball_pack_kernel<T><<<g, BLOCK, 0, (hipStream_t)stream>>>(plans, perm, (const T4*)rows4, (const T*)normals, m, Pm, bpc, (T4*)w.nrm4, w.inv);
    });
    return launch_status();
}

int dicp_fpfh_ball_spfh(int dtype, const void* plans, const uint64_t* keys, const int32_t* perm, const void* rows4, int N, int m, double radius,
                        void* workspace, size_t workspace_bytes, int32_t* spfh, unsigned long long* visited, void* stream) {
    if (!plans || !keys || !perm || !rows4 || !workspace) return DICP_ERR_NULL;
    int rc = fpfh_ball_check(dtype, N, m, radius, workspace_bytes);
    if (rc) return rc;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(plans, 8) || misaligned(keys, 8) || misaligned(perm, 4) || misaligned(rows4, 4 * ts) ||
        misaligned(spfh, 4) || misaligned(visited, 8))
        return DICP_ERR_ALIGN;
    const int Pm = ball_slots(m), bpc = (Pm + WAVE - 1) / WAVE;
    const unsigned g = (unsigned)N * (unsigned)bpc;
    const Workspace w = carve(workspace, dtype, N, m);
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        using T4 = typename V4<T>::type;
        fpfh_ball_spfh_kernel<T><<<g, WAVE, 0, (hipStream_t)stream>>>(plans, keys, perm, (const T4*)rows4, (const T4*)w.nrm4, m, Pm, bpc, radius, w.table,
                                                                      spfh, visited);
    });
    return launch_status();
}

int dicp_fpfh_ball_combine(int dtype, const void* plans, const uint64_t* keys, const int32_t* perm, const void* rows4, const void* at, int at64, int q,
                           int N, int m, double radius, const void* workspace, size_t workspace_bytes, void* out, unsigned long long* visited,
                           void* stream) {
    if (!plans || !keys || !perm || !rows4 || !workspace || !out) return DICP_ERR_NULL;
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (at64 != 0 && at64 != 1) return DICP_ERR_ENUM;
    int rc = fpfh_ball_check(dtype, N, m, radius, workspace_bytes);
    if (rc) return rc;
    if (at ? (q < 1 || (size_t)N * (size_t)q >= ((size_t)1 << 31)) : q != 0) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(workspace, 256) || misaligned(plans, 8) || misaligned(keys, 8) || misaligned(perm, 4) || misaligned(rows4, 4 * ts) ||
        misaligned(at, at64 ? 8 : 4) || misaligned(out, ts) || misaligned(visited, 8))
        return DICP_ERR_ALIGN;
    const int Pm = ball_slots(m), bpc = ((at ? q : Pm) + WAVE - 1) / WAVE;
    const unsigned g = (unsigned)N * (unsigned)bpc;
    const Workspace w = carve(workspace, dtype, N, m);
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        using T4 = typename V4<T>::type;
        if (at && at64)
            fpfh_ball_combine_kernel<T, int64_t><<<g, WAVE, 0, (hipStream_t)stream>>>(plans, keys, perm, (const T4*)rows4, (const int64_t*)at, q, m, Pm, bpc,
                                                                                      radius, w.table, w.inv, (T*)out, visited);
        else
            fpfh_ball_combine_kernel<T, int32_t><<<g, WAVE, 0, (hipStream_t)stream>>>(plans, keys, perm, (const T4*)rows4, (const int32_t*)at, q, m, Pm, bpc,
                                                                                      radius, w.table, w.inv, (T*)out, visited);
    });
    return launch_status();
}
