// Second-order spatial compatibility of correspondences and seeded consensus (dicp_amd/match.py: second_order_compatibility /
// prune_correspondences(order=2) / consensus_correspondences): the per-element rules of csrc/compat2.hip.
//
// Plain inline C++, included by the HIP kernels and by a TEST-ONLY g++ build (tests/test_compat2_host.py) that runs the same lines in a
// serial loop and holds them to the numpy restatement tests/compat2_ref.py.
//
// The live pairs, their packing and the relation are dicp_compat.h's (compat_pair<T>); the rules continue its numbering.
//   6  adjacency: W = ceil(n / 64) words of 64 bits per row; bit q % 64 of word q / 64 of row p (from the least significant bit) is 1 iff
//      p < P, q < P, p != q and the two are compatible; every other bit is 0.  Symmetric bit for bit, as the relation is.
//   7  common(p, q) = sum_w popcount(adj[p, w] & adj[q, w]);  S(p, q) = common(p, q) where bit (p, q) is set, 0 elsewhere;
//      degree2_p = sum_q S(p, q), an int64: twice the triangles through p.
//   8  rank2_p = the number of q below P with degree2_q > degree2_p, or degree2_q == degree2_p and q < p (on the integers).
//      score2_p = T(degree2_p) / T(max_q degree2_q), 0 where the maximum is 0 (the conversions go through double: exact below 2^53).
//   9  hypothesis h < min(seeds, P) is the pair s with rank2_s == h; its members are s, then the first min(members - 1, #{q : S(s, q) > 0})
//      positions q in the order (S(s, q) descending, q ascending) -- the descending order of key = S 2^32 + (2^32 - 1 - q).
//  10  the pose of a member list: the 18 Kabsch sums in double from 0, ransac_add_pair in member order, kabsch_forward, one rounding to T
//      (ransac_fit's closed form over a list).  Fewer than three members (S(s, .) has either no positive entry or at least two: a common
//      neighbour of s and q is itself a q' with S(s, q') > 0 -- so this is degree2_s == 0) or h >= P: the identity, as a cloud without
//      hypotheses gets from RANSAC.  Such hypotheses rank behind every real one, and their counts are zeroed before the choice.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dicp_compat.h"
#include "dicp_ransac.h"

namespace dicp {

constexpr int COMPAT2_N_MAX = 1 << 20;          // rows per cloud: degree2 <= n^2 = 2^40 stays exact in double
constexpr int COMPAT2_MEMBERS_MIN = 3;
constexpr int COMPAT2_MEMBERS_MAX = 32;

DICP_HD int compat2_words(int n) { return (n + 63) >> 6; }

// rule 6: the bit of (p, q)
DICP_HD bool compat2_bit(bool live_p, bool live_q, bool same, bool compatible) { return live_p && live_q && !same && compatible; }

DICP_HD int compat2_popc(uint64_t v) { return __builtin_popcountll(v); }

// rule 7: common(p, q) over the W words of two rows
DICP_HD int32_t compat2_common(const uint64_t* rp, const uint64_t* rq, int W) {
    int32_t c = 0;
    for (int w = 0; w < W; ++w) c += compat2_popc(rp[w] & rq[w]);
    return c;
}

DICP_HD bool compat2_has(const uint64_t* row, int q) { return (row[q >> 6] >> (q & 63)) & 1u; }

// rule 8: does (dq, q) come before (dp, p)?  The larger degree2, then the lower position
DICP_HD bool compat2_before(int64_t dq, int q, int64_t dp, int p) { return dq > dp || (dq == dp && q < p); }

template <typename T>
DICP_HD T compat2_score(int64_t d, int64_t dmax) {
    if (dmax <= 0) return T(0);
    return compat_div<T>((T)(double)d, (T)(double)dmax);
}

// rule 9: the key of candidate q with S > 0; a larger key comes first; 0 is no candidate
DICP_HD uint64_t compat2_key(int32_t S, int q) { return ((uint64_t)(uint32_t)S << 32) | (uint64_t)(0xffffffffu - (uint32_t)q); }
DICP_HD int32_t compat2_key_q(uint64_t key) { return (int32_t)(0xffffffffu - (uint32_t)(key & 0xffffffffu)); }

template <typename T>
DICP_HD void compat2_identity(T (&pose)[12]) {
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = (k < 9 && k % 4 == 0) ? T(1) : T(0);
}

// rule 10: the sums of a member list, in member order
template <typename T>
DICP_HD void compat2_sums(const T* pairs, const int32_t* members, int count, double (&acc)[NKAB]) {
#pragma unroll
    for (int i = 0; i < NKAB; ++i) acc[i] = 0.0;
    for (int k = 0; k < count; ++k) ransac_add_pair<T>(acc, pairs + (size_t)members[k] * RANSAC_ROW);
}

template <typename T>
DICP_HD void compat2_fit(const T* pairs, const int32_t* members, int count, T (&pose)[12]) {
    if (count < COMPAT2_MEMBERS_MIN) { compat2_identity<T>(pose); return; }
    double acc[NKAB], C[9], r[3], save[KAB_SAVE];
    compat2_sums<T>(pairs, members, count, acc);
    kabsch_forward(acc, C, r, save);
#pragma unroll
    for (int i = 0; i < 9; ++i) pose[i] = (T)C[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) pose[9 + i] = (T)r[i];
}

}  // namespace dicp
