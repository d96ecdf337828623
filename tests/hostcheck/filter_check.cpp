// TEST-ONLY host build of dicp_amd/csrc/dicp_filter.h (g++, no GPU): the rules of the statistical outlier filter that the HIP kernels
// execute, for tests/test_filter_host.py.  Never loaded by dicp_amd.
//
// variant 0 is the header's rule.  The others are WRONG rules, written out here, which the comparison with tests/filter_ref.py must
// refuse: 1 plain sequential sums, 2 a population variance, 3 `<` for `<=`, 4 the self slot not skipped, 5 the square fused into the
// addition.  Variant 6 is the header's rule run the way the kernels run it -- as many rounds of partials as a cloud of m valid rows
// would need, whatever V is -- and must agree with variant 0.
#include <cmath>
#include <vector>

#include "../../dicp_amd/csrc/dicp_filter.h"

using namespace dicp;

namespace {

enum { RIGHT = 0, SEQUENTIAL = 1, POPULATION = 2, STRICT = 3, KEEP_SELF = 4, FUSED = 5, KERNEL_ROUNDS = 6 };

double plain_sum(const double* v, int64_t len) {
    double s = 0.0;
    for (int64_t i = 0; i < len; ++i) s = s + v[i];
    return s;
}

// `levels` rounds of partials with the length taken from `len`, as the level kernels do: -> the one value left
double rounds_sum(std::vector<double> v, int64_t len, int levels) {
    for (int l = 0; l < levels; ++l) {
        const int64_t nc = filter_chunks(len) > 0 ? filter_chunks(len) : 1;     // (partial 0 is always written)
        std::vector<double> out((size_t)nc);
        for (int64_t j = 0; j < nc; ++j) {
            int64_t rest = len - j * FILTER_CHUNK;
            if (rest < 0) rest = 0;
            out[(size_t)j] = filter_chunk_sum(v.data() + j * FILTER_CHUNK, (int)(rest < FILTER_CHUNK ? rest : FILTER_CHUNK));
        }
        v.swap(out);
        len = filter_chunks(len);
    }
    return v[0];
}

template <typename T>
double row_mean(const T* d2, const int64_t* idx, int64_t i, int k, int variant, int* cnt) {
    if (variant != KEEP_SELF) return outlier_row_mean<T>(d2, idx, i, k, cnt);
    double s = 0.0;
    int n = 0;
    for (int q = 0; q <= k && n < k; ++q) {
        if (idx[q] < 0) continue;
        s = s + filter_sqrt((double)d2[q]);
        ++n;
    }
    *cnt = n;
    return n ? s / (double)n : (double)INFINITY;
}

double total(std::vector<double>& v, int m, int variant) {
    const int64_t len = (int64_t)v.size();
    if (variant == SEQUENTIAL) return plain_sum(v.data(), len);
    if (variant == KERNEL_ROUNDS) { v.resize((size_t)len + FILTER_CHUNK, 0.0); return rounds_sum(v, len, filter_levels(m)); }
    return filter_sum64(v.data(), len);
}

template <typename T>
void cloud(const T* d2, const int64_t* idx, int m, int rows, int k, double std_ratio, int variant, double* md, double* stats, uint8_t* mask) {
    std::vector<double> vals;
    std::vector<uint8_t> valid((size_t)m, 0);
    for (int i = 0; i < m; ++i) {
        int cnt = 0;
        md[i] = (double)INFINITY;
        if (i < rows) md[i] = row_mean<T>(d2 + (size_t)i * (k + 1), idx + (size_t)i * (k + 1), i, k, variant, &cnt);
        valid[(size_t)i] = cnt > 0;
        if (cnt > 0) vals.push_back(md[i]);
    }
    const int64_t V = (int64_t)vals.size();
    std::vector<double> a(vals);
    const double mean = outlier_mean(total(a, m, variant), V);
    // the first round squares the deviations; the partials go on as a plain list
    std::vector<double> part;
    if (variant == SEQUENTIAL) {
        for (int64_t i = 0; i < V; ++i) { const double t = vals[(size_t)i] - mean; const double q = t * t; part.push_back(q); }
    } else {
        for (int64_t j = 0; j * FILTER_CHUNK < V || j == 0; ++j) {
            int64_t rest = V - j * FILTER_CHUNK;
            const int n = (int)(rest < 0 ? 0 : (rest < FILTER_CHUNK ? rest : FILTER_CHUNK));
            const double* v = vals.data() + j * FILTER_CHUNK;
            if (variant == FUSED) {
                double s = 0.0;
                for (int i = 0; i < n; ++i) { const double t = v[i] - mean; s = std::fma(t, t, s); }
                part.push_back(s);
            } else {
                part.push_back(filter_chunk_sqdev(v, n, mean));
            }
        }
    }
    double sum_sq;
    if (variant == KERNEL_ROUNDS) {
        const int64_t len = (int64_t)part.size();
        part.resize((size_t)len + FILTER_CHUNK, 0.0);
        sum_sq = rounds_sum(part, filter_chunks(V), filter_levels(m) - 1);
    } else {
        sum_sq = total(part, m, variant);
    }
    if (variant == POPULATION) {
        double sd = 0.0;
        if (V >= 2) sd = filter_sqrt(sum_sq / (double)V);
        const double p = std_ratio * sd;
        stats[0] = mean; stats[1] = sd; stats[2] = mean + p;
    } else {
        outlier_stats(mean, sum_sq, V, std_ratio, stats);
    }
    for (int i = 0; i < m; ++i)
        mask[i] = variant == STRICT ? (valid[(size_t)i] && md[i] < stats[2]) : outlier_keep(valid[(size_t)i] != 0, md[i], stats[2]);
}

}  // namespace

extern "C" {

// SELECT_TILE, SELECT_SCAN_THREADS, FILTER_CHUNK, OUTLIER_K_MIN, OUTLIER_K_MAX
void fc_constants(int32_t* out) {
    out[0] = SELECT_TILE; out[1] = SELECT_SCAN_THREADS; out[2] = FILTER_CHUNK; out[3] = OUTLIER_K_MIN; out[4] = OUTLIER_K_MAX;
}
int fc_levels(int64_t cap) { return filter_levels(cap); }
int64_t fc_level_len(int64_t len, int levels) { return filter_level_len(len, levels); }

double fc_sum64(const double* v, int64_t len, int variant) {
    std::vector<double> a(v, v + len);
    if (variant == SEQUENTIAL) return plain_sum(a.data(), len);
    if (variant == KERNEL_ROUNDS) { a.resize((size_t)len + FILTER_CHUNK, 0.0); return rounds_sum(a, len, filter_levels(len > 0 ? len : 1) + 1); }
    return filter_sum64(a.data(), len);
}

void fc_row_means_f32(const float* d2, const int64_t* idx, int m, int k, int variant, double* md, int32_t* cnt) {
    for (int i = 0; i < m; ++i) { int c; md[i] = row_mean<float>(d2 + (size_t)i * (k + 1), idx + (size_t)i * (k + 1), i, k, variant, &c); cnt[i] = c; }
}
void fc_row_means_f64(const double* d2, const int64_t* idx, int m, int k, int variant, double* md, int32_t* cnt) {
    for (int i = 0; i < m; ++i) { int c; md[i] = row_mean<double>(d2 + (size_t)i * (k + 1), idx + (size_t)i * (k + 1), i, k, variant, &c); cnt[i] = c; }
}
void fc_cloud_f32(const float* d2, const int64_t* idx, int m, int rows, int k, double std_ratio, int variant, double* md, double* stats, uint8_t* mask) {
    cloud<float>(d2, idx, m, rows, k, std_ratio, variant, md, stats, mask);
}
void fc_cloud_f64(const double* d2, const int64_t* idx, int m, int rows, int k, double std_ratio, int variant, double* md, double* stats, uint8_t* mask) {
    cloud<double>(d2, idx, m, rows, k, std_ratio, variant, md, stats, mask);
}

}
