// The deterministic gradient of the surface normals (estimate_normals with deterministic=True): the per-element rules of
// csrc/normals_det.hip, on the inverted index of the neighbour tensor (csrc/dicp_inverse.h).
//
// Plain inline C++ templated on the scalar T and the index type I, included by the HIP kernels and by a TEST-ONLY g++ build
// (tests/test_normals_det_host.py) that runs the same lines in a serial loop and holds them to the numpy restatement tests/normals_det_ref.py.
//
// Every row of a cloud has a RECORD of NRM_REC = 13 doubles, written by the records pass from the query's eigen-system:
//   [0..6) G6 = dL/dC symmetrised (nrm_grad_cov), [6..9) mu, [9..12) p = the row's coordinates (exact in double), [12] f = 2 / k_eff,
//   or f = 0 when the query contributes nothing (k_eff < 3, both cotangents zero or absent, eigenvalues not separated, zero trace).
// Row j receives, per component a in 0..2, the sum over its list (the slots q = i k + o with nbr[i, o] = j, in ascending q) of
//   d_c = ((double)y_c - (double)p_c) - mu_c,   t_a = (T)(f * ((G_a0 * d_0 + G_a1 * d_1) + G_a2 * d_2))
// with y = record j's p and G, mu, p, f = record i's: every product and every sum rounded once in double (a statement each, so that
// -ffp-contract=on cannot fuse them), then once to T.  An entry whose query has f = 0 has no term; its position still counts.  The
// order of summation is dicp_inverse.h's: chunks of GROUP_DET_CHUNK list positions, each summed from +0 by plain additions in T, the
// partials added in order to a total that starts at +0, a list of at most one chunk giving its partial itself.  The walk never leaves
// its arrays whatever offsets / slots / the index hold: det_list's clamps and det_entry's check.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dicp_inverse.h"

namespace dicp {

constexpr int NRM_REC = 13;
enum { NRM_REC_G = 0, NRM_REC_MU = 6, NRM_REC_P = 9, NRM_REC_F = 12 };

// One cloud's arrays: rec (m, NRM_REC) the records, idx (m, k) the neighbours as original rows; rows: the cloud's row count
template <typename I>
struct NrmDetCloud {
    const double* rec;
    const I* idx;
    int m, k, rows;
};

// a query's record: G6 and mu as given, p and f; `on` false leaves G6 = mu = 0 and f = 0 (the query contributes nothing)
DICP_HD void nrm_det_record(double* R, bool on, const double* G6, const double* mu, const double* p, int k_eff) {
    for (int e = 0; e < 6; ++e) R[NRM_REC_G + e] = on ? G6[e] : 0.0;
    for (int e = 0; e < 3; ++e) R[NRM_REC_MU + e] = on ? mu[e] : 0.0;
    for (int e = 0; e < 3; ++e) R[NRM_REC_P + e] = p[e];
    R[NRM_REC_F] = on ? 2.0 / k_eff : 0.0;
}

// the three terms of one entry: R the query's record, y the row's coordinates
template <typename T>
DICP_HD void nrm_det_term(const double* R, const double* y, T* t) {
    double d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double e = y[c] - R[NRM_REC_P + c];
        d[c] = e - R[NRM_REC_MU + c];
    }
    const double* G = R + NRM_REC_G;
    const double g[3][3] = {{G[0], G[1], G[2]}, {G[1], G[3], G[4]}, {G[2], G[4], G[5]}};
    const double f = R[NRM_REC_F];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double p0 = g[a][0] * d[0];
        const double p1 = g[a][1] * d[1];
        const double s1 = p0 + p1;
        const double p2 = g[a][2] * d[2];
        const double s2 = s1 + p2;
        const double r = f * s2;
        t[a] = (T)r;
    }
}

// part[0..3) = part + the terms of list positions [e0, e1) of row j, in order; y: the row's three coordinates.  NRM_DET_ILP entries at
// a time: their loads (the slot number, then the index, then the query's 104-byte record) do not depend on one another, so they are in
// flight together; an entry that is not taken reads slot 0 and record 0 of the cloud instead (in range: m k >= 1) and its term is
// dropped.  The additions stay one per taken entry, in list order.
constexpr int NRM_DET_ILP = 4;
template <typename T, typename I>
DICP_HD void nrm_det_entries(const NrmDetCloud<I>& a, const int32_t* slots, int j, const double* y, int e0, int e1, T* part) {
    const int nk = a.m * a.k;
    for (int e = e0; e < e1; e += e1 - e > NRM_DET_ILP ? NRM_DET_ILP : e1 - e) {
        T t[NRM_DET_ILP][3];
        bool has[NRM_DET_ILP];
#pragma unroll
        for (int u = 0; u < NRM_DET_ILP; ++u) {
            const bool in_list = u < e1 - e;
            const int32_t q = slots[in_list ? e + u : e];
            const bool in_range = (uint32_t)q < (uint32_t)nk;
            const int32_t qq = in_range ? q : 0;
            const bool ok = in_list && in_range && det_entry<I>(qq, nk, a.idx, a.rows, j);
            const double* R = a.rec + (size_t)(qq / a.k) * NRM_REC;
            has[u] = ok && !(R[NRM_REC_F] == 0.0);
            nrm_det_term<T>(R, y, t[u]);
        }
#pragma unroll
        for (int u = 0; u < NRM_DET_ILP; ++u) {
            if (!has[u]) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) part[c] = part[c] + t[u][c];
        }
    }
}

DICP_HD int nrm_det_chunks(int lo, int hi) { return (hi - lo) / GROUP_DET_CHUNK + ((hi - lo) % GROUP_DET_CHUNK != 0); }

// out[0..3) = the gradient of row j's coordinates over the list [lo, hi) (det_list's)
template <typename T, typename I>
DICP_HD void nrm_det_row_sum(const NrmDetCloud<I>& a, const int32_t* slots, int j, const double* y, int lo, int hi, T* out) {
    T total[3] = {T(0), T(0), T(0)}, part[3] = {T(0), T(0), T(0)};
    const int chunks = nrm_det_chunks(lo, hi);
    for (int ch = 0; ch < chunks; ++ch) {
        if (det_chunk_start(ch * GROUP_DET_CHUNK)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) det_flush<T>(total[c], part[c]);
        }
        const int e0 = lo + ch * GROUP_DET_CHUNK;           // (< hi <= m k < 2^31)
        nrm_det_entries<T, I>(a, slots, j, y, e0, hi - e0 > GROUP_DET_CHUNK ? e0 + GROUP_DET_CHUNK : hi, part);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = det_finish<T>(total[c], part[c], hi - lo);
}

// row j of a cloud: out[0..3) from its record and its list, +0 for a row at or past the row count
template <typename T, typename I>
DICP_HD void nrm_det_row(const NrmDetCloud<I>& a, const int32_t* offsets, const int32_t* slots, int j, T* out) {
    out[0] = out[1] = out[2] = T(0);
    if (j >= a.rows) return;
    const double* Rj = a.rec + (size_t)j * NRM_REC;
    const double y[3] = {Rj[NRM_REC_P], Rj[NRM_REC_P + 1], Rj[NRM_REC_P + 2]};
    int lo, hi;
    det_list(offsets, j, a.m * a.k, lo, hi);
    nrm_det_row_sum<T, I>(a, slots, j, y, lo, hi, out);
}

}  // namespace dicp
