// TEST-ONLY host build of dicp_amd/csrc/dicp_compat2.h (g++, no GPU): the adjacency bits, the masked common counts, degree2, rank2,
// score2, the member lists by their keys and the fit of a list -- the lines the HIP kernels execute -- run in a serial loop over one cloud's
// packed pairs, for tests/test_compat2_host.py.  Never loaded by dicp_amd.
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "../../dicp_amd/csrc/dicp_compat2.h"

using namespace dicp;

namespace {

// adj (n, W) and the degree (n) of one cloud's P packed pairs
template <typename T>
void bits(const T* pairs, int P, int n, double threshold, double min_length, uint64_t* adj, int32_t* degree) {
    const T thr = compat_thr<T>(threshold), L = compat_thr<T>(min_length);
    const int W = compat2_words(n);
    for (int p = 0; p < n; ++p) {
        int32_t deg = 0;
        for (int w = 0; w < W; ++w) {
            uint64_t word = 0;
            for (int b = 0; b < 64; ++b) {
                const int q = w * 64 + b;
                bool ok = false;
                if (p < P && q < P) {
                    const T* a = pairs + (size_t)p * COMPAT_ROW;
                    const T* c = pairs + (size_t)q * COMPAT_ROW;
                    ok = compat_pair<T>(a[0], a[1], a[2], a[3], a[4], a[5], c[0], c[1], c[2], c[3], c[4], c[5], thr, L);
                }
                word |= compat2_bit(p < P, q < P, q == p, ok) ? ((uint64_t)1 << b) : 0;
            }
            adj[(size_t)p * W + w] = word;
            deg += compat2_popc(word);
        }
        degree[p] = deg;
    }
}

// S (P, P) and degree2 (P) from the bits
void second(const uint64_t* adj, int P, int n, int32_t* S, int64_t* degree2) {
    const int W = compat2_words(n);
    for (int p = 0; p < P; ++p) {
        int64_t d = 0;
        for (int q = 0; q < P; ++q) {
            const int32_t s = compat2_has(adj + (size_t)p * W, q) ? compat2_common(adj + (size_t)p * W, adj + (size_t)q * W, W) : 0;
            S[(size_t)p * P + q] = s;
            d += s;
        }
        degree2[p] = d;
    }
}

void rank_of(const int64_t* degree2, int P, int32_t* rank) {
    for (int p = 0; p < P; ++p) {
        int32_t r = 0;
        for (int q = 0; q < P; ++q) r += compat2_before(degree2[q], q, degree2[p], p) ? 1 : 0;
        rank[p] = r;
    }
}

template <typename T>
void score_of(const int64_t* degree2, int P, T* score2) {
    int64_t mx = 0;
    for (int p = 0; p < P; ++p) mx = degree2[p] > mx ? degree2[p] : mx;
    for (int p = 0; p < P; ++p) score2[p] = compat2_score<T>(degree2[p], mx);
}

// lists (seeds, members): the seed of rank h, then the candidates in descending key order
void members_of(const uint64_t* adj, int P, int n, const int32_t* rank2, int seeds, int members, int32_t* lists) {
    const int W = compat2_words(n);
    for (int h = 0; h < seeds; ++h) {
        int32_t* out = lists + (size_t)h * members;
        for (int k = 0; k < members; ++k) out[k] = -1;
        if (h >= P) continue;
        int s = -1;
        for (int p = 0; p < P; ++p)
            if (rank2[p] == h) s = p;
        const uint64_t* rs = adj + (size_t)s * W;
        std::vector<uint64_t> keys;
        for (int q = 0; q < P; ++q)
            if (compat2_has(rs, q)) {
                const int32_t S = compat2_common(rs, adj + (size_t)q * W, W);
                if (S > 0) keys.push_back(compat2_key(S, q));
            }
        std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
        out[0] = s;
        for (int k = 1; k < members && k - 1 < (int)keys.size(); ++k) out[k] = compat2_key_q(keys[(size_t)k - 1]);
    }
}

// sums (seeds, 18) and poses (seeds, 12) of the lists
template <typename T>
void fit(const T* pairs, const int32_t* lists, int seeds, int members, double* sums, T* poses) {
    for (int h = 0; h < seeds; ++h) {
        const int32_t* lst = lists + (size_t)h * members;
        int count = 0;
        while (count < members && lst[count] >= 0) ++count;
        double acc[NKAB];
        compat2_sums<T>(pairs, lst, count, acc);
        for (int i = 0; i < NKAB; ++i) sums[(size_t)h * NKAB + i] = acc[i];
        T pose[12];
        compat2_fit<T>(pairs, lst, count, pose);
        for (int i = 0; i < 12; ++i) poses[(size_t)h * 12 + i] = pose[i];
    }
}

}  // namespace

extern "C" {

int c2_n_max() { return COMPAT2_N_MAX; }
int c2_members_max() { return COMPAT2_MEMBERS_MAX; }
int c2_words(int n) { return compat2_words(n); }
void c2_bits_f32(const float* pairs, int P, int n, double thr, double L, uint64_t* adj, int32_t* degree) { bits<float>(pairs, P, n, thr, L, adj, degree); }
void c2_bits_f64(const double* pairs, int P, int n, double thr, double L, uint64_t* adj, int32_t* degree) { bits<double>(pairs, P, n, thr, L, adj, degree); }
void c2_second(const uint64_t* adj, int P, int n, int32_t* S, int64_t* degree2) { second(adj, P, n, S, degree2); }
void c2_rank(const int64_t* degree2, int P, int32_t* rank) { rank_of(degree2, P, rank); }
void c2_score_f32(const int64_t* degree2, int P, float* score2) { score_of<float>(degree2, P, score2); }
void c2_score_f64(const int64_t* degree2, int P, double* score2) { score_of<double>(degree2, P, score2); }
void c2_members(const uint64_t* adj, int P, int n, const int32_t* rank2, int seeds, int members, int32_t* lists) {
    members_of(adj, P, n, rank2, seeds, members, lists);
}
void c2_fit_f32(const float* pairs, const int32_t* lists, int seeds, int members, double* sums, float* poses) { fit<float>(pairs, lists, seeds, members, sums, poses); }
void c2_fit_f64(const double* pairs, const int32_t* lists, int seeds, int members, double* sums, double* poses) { fit<double>(pairs, lists, seeds, members, sums, poses); }

}
