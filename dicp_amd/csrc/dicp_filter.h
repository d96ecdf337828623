// The rules of the outlier filters (dicp_amd/filter.py, csrc/filter.hip): the geometry of the mask compaction and, per row and per
// cloud, the arithmetic of the statistical filter.
//
// Plain inline C++, included by the HIP kernels and by a TEST-ONLY g++ build (tests/test_filter_host.py) that holds these rules
// to numpy (tests/filter_ref.py) bit for bit on a CPU box with no GPU.
//
// Compaction (select_rows): row r of cloud b is kept when r < rows[b] and mask[b, r]; kept rows keep their order.  The kernels work
// on tiles of SELECT_TILE rows that never straddle two clouds.
//
// Statistical filter, everything in double, for the (k + 1)-slot search result (d2, idx) of a cloud against itself:
//   live slots   row i walks its k + 1 slots in order, skips every slot whose idx is i itself and every empty one (idx < 0), and takes
//                the first k that remain: cnt_i of them
//   md_i         (sum of sqrt((double)d2) over the live slots, in slot order from +0) / cnt_i; +inf when cnt_i = 0: the row is invalid,
//                takes no part in the statistics and is dropped
//   sum64        a list of at most FILTER_CHUNK values is added sequentially from +0; a longer one is cut into consecutive chunks of
//                FILTER_CHUNK, each summed that way, and sum64 is applied to the list of the partials (a radix-64 tree)
//   statistics   over the cloud's V valid rows in row order: mean = sum64(md) / V; var = sum64(t t) / (V - 1) with t = md - mean and
//                the product rounded on its own; std = sqrt(var), 0 when V < 2; thr = mean + (std_ratio std), the product rounded first
//                (V = 0: mean and thr are 0 / 0 = NaN)
//   decision     keep row i when cnt_i > 0 and md_i <= thr
// The build contracts a * b + c only inside ONE expression (-ffp-contract=on): every product that must be rounded on its own is a
// statement of its own below.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dicp_math.h"

namespace dicp {

constexpr int SELECT_TILE = 1024;          // rows per tile of the compaction kernels
constexpr int SELECT_SCAN_THREADS = 256;   // threads of the per-cloud scan of the tile counts: tiles per pass
constexpr int FILTER_CHUNK = 64;           // the radix of sum64
constexpr int OUTLIER_K_MIN = 1, OUTLIER_K_MAX = 31;
constexpr int OUTLIER_STATS = 3;           // mean, std, thr

// The double root of the filter.  IEEE sqrt on the host; the device library's is correctly rounded too (the GPU tests compare the
// row means bit for bit with numpy's).
DICP_HD double filter_sqrt(double x) { return sqrt(x); }

// -> md_i and *cnt: d2 / idx are row i's k + 1 slots, `self` is i
template <typename T>
DICP_HD double outlier_row_mean(const T* d2, const int64_t* idx, int64_t self, int k, int* cnt) {
    double s = 0.0;
    int n = 0;
    for (int q = 0; q <= k && n < k; ++q) {
        const int64_t j = idx[q];
        if (j < 0 || j == self) continue;
        s = s + filter_sqrt((double)d2[q]);
        ++n;
    }
    *cnt = n;
    return n ? s / (double)n : (double)INFINITY;
}

// chunks of a list of len values; the length of the list after `levels` rounds of partials
DICP_HD int64_t filter_chunks(int64_t len) { return (len + FILTER_CHUNK - 1) / FILTER_CHUNK; }
DICP_HD int64_t filter_level_len(int64_t len, int levels) {
    for (int l = 0; l < levels; ++l) len = filter_chunks(len);
    return len;
}
// rounds of partials after which a list of at most `cap` values has become ONE value (at least one round)
DICP_HD int filter_levels(int64_t cap) {
    int l = 1;
    for (cap = filter_chunks(cap); cap > 1; cap = filter_chunks(cap)) ++l;
    return l;
}

// one chunk (n <= FILTER_CHUNK values): sequentially from +0.  A list of one partial x gives 0 + x = x, so a round of partials more
// than the list needs changes nothing.
DICP_HD double filter_chunk_sum(const double* v, int n) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s = s + v[i];
    return s;
}
// the same over (v - mean)^2, each square rounded before it is added
DICP_HD double filter_chunk_sqdev(const double* v, int n, double mean) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
        const double t = v[i] - mean;
        const double q = t * t;
        s = s + q;
    }
    return s;
}

// sum64 of v[0 .. len), in place: v is overwritten by the partials.  (The kernels run the same rounds, one launch each.)
DICP_HD double filter_sum64(double* v, int64_t len) {
    while (len > FILTER_CHUNK) {
        const int64_t nc = filter_chunks(len);
        for (int64_t j = 0; j < nc; ++j) {
            const int64_t rest = len - j * FILTER_CHUNK;
            v[j] = filter_chunk_sum(v + j * FILTER_CHUNK, (int)(rest < FILTER_CHUNK ? rest : FILTER_CHUNK));
        }
        len = nc;
    }
    return filter_chunk_sum(v, (int)len);
}

DICP_HD double outlier_mean(double sum_md, int64_t V) { return sum_md / (double)V; }

// stats[0..3) = mean, std, thr from the two sums of a cloud with V valid rows
DICP_HD void outlier_stats(double mean, double sum_sq, int64_t V, double std_ratio, double* stats) {
    double sd = 0.0;
    if (V >= 2) {
        const double var = sum_sq / (double)(V - 1);
        sd = filter_sqrt(var);
    }
    const double p = std_ratio * sd;
    stats[0] = mean;
    stats[1] = sd;
    stats[2] = mean + p;
}

DICP_HD bool outlier_keep(bool valid, double md, double thr) { return valid && md <= thr; }

}  // namespace dicp
