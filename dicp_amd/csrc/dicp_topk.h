// The exact k-nearest-neighbour walk over a cloud sorted by raw x, shared by csrc/normals.hip (queries are rows of the cloud they walk)
// and csrc/knn_points.hip (queries from another cloud).
//
// Plain inline C++ templated on the scalar T, the row type (anything with .x .y .z: float4 / double4 on the device) and the accessors,
// included by the HIP kernels and by a TEST-ONLY g++ build (tests/test_knn_points_host.py) that holds the walk to a numpy brute force.
//
// d2(p, y) = (xx + yy) + zz with dx = y.x - p.x, xx = dx * dx, ... as separate statements: -ffp-contract=on fuses only inside one
// expression, so these are the roundings numpy's float32 / float64 arithmetic makes.
// The walk: the rows of one cloud sorted ascending in x (NaN last), a query p and a split: every row left of `hi` has x <= p.x and every
// row from `hi` on has x >= p.x (the lower bound of p.x; for a query that is row s of the cloud itself, s with lo = s - 1, hi = s + 1).
// Two cursors move outward, the side with the smaller x gap first, and the walk stops once gap * gap > the k-th best d2 so far.
// Exact, query a row or not: the gap of the row on the right is fl(y.x - p.x) = dx; on the left it is fl(p.x - y.x) = -dx exactly
// (round-to-nearest is symmetric), so gap * gap is that row's xx; d2 = fl(fl(xx + yy) + zz) >= xx for non-negative terms under monotone
// rounding; every row further out on that side has a gap at least as large (fl(a - b) is monotone in a), and the side not taken has a gap
// at least as large as well.  So no row beyond the stop has d2 <= the bound; ties at the k-th d2 are still examined, and the (d2, index)
// order holds.  A NaN gap never stops the walk (the comparison is false) and a NaN or +inf d2 never enters the list (the empty tail is
// +inf with index -1, and every row index is >= 0): a query with a non-finite coordinate walks every row and gets no neighbours.
#pragma once
#include <type_traits>

#include "dicp_math.h"

namespace dicp {

// (d2, index) order
template <typename T>
DICP_HD bool topk_before(T da, int ia, T db, int ib) { return da < db || (da == db && ia < ib); }

template <typename T, typename P, typename Y>
DICP_HD T topk_d2(const P& p, const Y& y) {
    const T dx = y.x - p.x;
    const T dy = y.y - p.y;
    const T dz = y.z - p.z;
    const T xx = dx * dx;
    const T yy = dy * dy;
    const T zz = dz * dz;
    return (xx + yy) + zz;
}

// The first of keys[0, n) that is not below x (keys ascending, NaN last); n when there is none, 0 for a NaN x
template <typename T>
DICP_HD int topk_lower_bound(const T* keys, int n, T x) {
    int lo = 0, len = n;
    while (len > 0) {
        const int h = len >> 1;
        if (keys[lo + h] < x) { lo += h + 1; len -= h + 1; }
        else len = h;
    }
    return lo;
}

// The k best (d2, original index) of the rows seen, with the sorted slot each came from: d / id / sl, register arrays of capacity K >= k
// (plain arrays the caller declares: kept in a struct, the same code held 50 % more VGPRs).  The list is entries K - k .. K - 1,
// ascending; the unused head is -inf (never beaten), the empty tail +inf with index and slot -1.  The insertion is unrolled over K, so
// K = 1 costs one comparison per row.
template <typename T, int K>
DICP_HD void topk_init(T (&d)[K], int (&id)[K], int (&sl)[K], int k) {
    const T inf = static_cast<T>(__builtin_huge_val());
#pragma unroll
    for (int i = 0; i < K; ++i) { d[i] = i < K - k ? -inf : inf; id[i] = -1; sl[i] = -1; }
}

// The list capacities the kernels are instantiated for: the smallest of 1, 4, 8, 16, 32 that holds k
inline int topk_kcap(int k) { return k == 1 ? 1 : (k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 16 ? 16 : 32))); }

// f(std::integral_constant<int, K>()) for K = topk_kcap(k): f is a generic lambda that launches the kernel instantiated for K; what it
// returns is returned.
template <typename F>
inline auto topk_with_kcap(int k, F&& f) {
    switch (topk_kcap(k)) {
        case 1: return f(std::integral_constant<int, 1>());
        case 4: return f(std::integral_constant<int, 4>());
        case 8: return f(std::integral_constant<int, 8>());
        case 16: return f(std::integral_constant<int, 16>());
        default: return f(std::integral_constant<int, 32>());
    }
}

// (The write-out of entries K - k .. K - 1 stays an inline loop in the three kernels: as a helper taking a per-entry callable it cost
// normals_knn_kernel<double, 16 / 32> and every ball_query_kernel 2 to 5 VGPRs, and ball_query_kernel<float, 8 / 32> a wave of occupancy.)

// The insertion as a callable ins(d2, j): row j of the sorted cloud at distance d2; orig(j) its original index, read only when d2 can
// enter.  (A lambda, not a forced-inline function: inlined by the optimiser in its own time, the walk kernels keep the registers of the
// hand-written form -- forced in early, 50 % more VGPRs at K = 32.)
template <typename T, int K, typename Orig>
DICP_HD auto topk_inserter(T (&d)[K], int (&id)[K], int (&sl)[K], const Orig& orig) {
    return [&d, &id, &sl, &orig](T d2, int j) {
        if (!(d2 <= d[K - 1])) return;
        const int o = orig(j);
        if (!topk_before(d2, o, d[K - 1], id[K - 1])) return;
#pragma unroll
        for (int i = K - 1; i > 0; --i) {
            const bool shift = topk_before(d2, o, d[i - 1], id[i - 1]);
            const bool put = !shift && (i == K - 1 || topk_before(d2, o, d[i], id[i]));
            d[i] = shift ? d[i - 1] : (put ? d2 : d[i]);
            id[i] = shift ? id[i - 1] : (put ? o : id[i]);
            sl[i] = shift ? sl[i - 1] : (put ? j : sl[i]);
        }
        if (topk_before(d2, o, d[0], id[0])) { d[0] = d2; id[0] = o; sl[0] = j; }
    };
}

// The two-cursor walk from the split (lo, hi) over the rows [0, mb) of a sorted cloud; row(j) returns row j (.x .y .z), ins the
// inserter of the list d.  Returns the number of rows visited.
template <typename T, int K, typename P, typename Row, typename Ins>
DICP_HD unsigned topk_walk(const T (&d)[K], const P& p, int lo, int hi, int mb, const Row& row, const Ins& ins) {
    unsigned steps = 0;
    bool cl = lo >= 0, ch = hi < mb;
    if (!cl && !ch) return 0;
    auto yl = row(cl ? lo : hi), yh = row(ch ? hi : lo);      // (a live side's row; the other is not read)
    while (cl || ch) {
        const T gl = p.x - yl.x, gh = yh.x - p.x;
        const bool left = cl && (!ch || gl <= gh);
        const T g = left ? gl : gh;
        const T g2 = g * g;
        if (g2 > d[K - 1]) break;                   // this side is the nearer one: the other is beyond the bound as well
        ++steps;
        if (left) { ins(topk_d2<T>(p, yl), lo); --lo; cl = lo >= 0; if (cl) yl = row(lo); }
        else      { ins(topk_d2<T>(p, yh), hi); ++hi; ch = hi < mb; if (ch) yh = row(hi); }
    }
    return steps;
}

}  // namespace dicp
