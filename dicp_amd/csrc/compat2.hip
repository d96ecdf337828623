// Second-order spatial compatibility and seeded consensus (dicp_compat2_bits, dicp_compat2_common, dicp_compat2_rank, dicp_compat2_seeds;
// dicp_amd/match.py).  The rules per element are csrc/dicp_compat2.h's, on top of csrc/dicp_compat.h's relation.  The input is the PACKED
// pair list of every cloud -- (N, n, 6) rows (x[0:3], y[0:3]) with the cloud's P live pairs first -- and P (N).
//
//   compat_bits_kernel    compat_pass_kernel's tile walk (a lane per row p, q broadcast from LDS tiles of C2_TILE rows), but the decisions of
//                         64 consecutive q are packed into one word instead of added; a lane keeps the tile's 8 words in registers and
//                         stores them together (one 64-byte line).  Rows and bits at or past P and the diagonal are zero by construction;
//                         workgroups past P store their rows of zeros as one contiguous range.  Also the int32 degree (the popcount of the
//                         row) and the zero of degree2.  The arithmetic of one first-order pass; n W words written.
//   compat_common_kernel  the hot path, a binary matrix product masked by its own operand: a workgroup takes C2_TP rows p x a chunk of C2_QC
//                         rows q of one cloud and walks the q in tiles of 64.  Per (p tile, q tile) the words of both are staged in LDS in
//                         chunks of C2_WC words, word-major ([word][row], rows padded to C2_LD so that the transposing stores spread over
//                         the banks and a lane's four consecutive rows are two 16-byte reads); a lane keeps a 4 x 4 tile of counts and adds
//                         popcount(a_i & b_j) -- two ANDs and two accumulating v_bcnt_u32_b32 per word pair.  The counts are masked by the
//                         bits (p, q) of the p rows' own word, summed over q per row, reduced over the 16 lanes that share the row and
//                         added to degree2 with one integer atomic per row and workgroup: order-independent.  Bound by the vector issue
//                         rate: 4 vector operations per word pair, n^2 W word pairs per cloud.
//   compat2_rank_kernel   compat_rank_kernel's loop over the int64 degree2: rank2, the cloud's maximum (every lane walks every q) and from
//                         it score2; the rows of rank below `seeds` are scattered into seedpos[cloud, rank] (ranks are a permutation: one
//                         writer each).
//   compat2_seed_kernel   a wave per (cloud, hypothesis): the wave walks the seed row's words (word i holds the bits of q = 64 i + lane, so
//                         the test of a whole word is uniform), a lane whose bit is set computes S(s, q) over the row's words, and keeps the
//                         best members - 1 keys (S, -q) in a sorted list of its own in LDS; the lists are merged by members - 1 wave maxima.
//                         Lane 0 then fits the list in double (kabsch_forward), as ransac_hyp_kernel's lanes do.
// The grids are sized by n (never by P: nothing is read back).  No float atomics anywhere: every output is bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dicp_common.h"
#include "dicp_compat2.h"

namespace {

constexpr int C2_TILE = 512;            // packed rows q per LDS tile of the bits and rank kernels: 8 words
constexpr int C2_TW = C2_TILE / 64;
constexpr int C2_TP = 64;               // rows of a p tile and of a q tile of the common kernel
constexpr int C2_WC = 32;               // words per LDS chunk
constexpr int C2_LD = C2_TP + 2;        // padded rows of a word's LDS line
constexpr int C2_QC = 1024;             // rows q per workgroup of the common kernel
constexpr int C2_KMAX = COMPAT2_MEMBERS_MAX - 1;

template <typename T> __device__ __forceinline__ T c2_nan();
template <> __device__ __forceinline__ float  c2_nan<float>()  { return __builtin_nanf(""); }
template <> __device__ __forceinline__ double c2_nan<double>() { return __builtin_nan(""); }

template <typename T>
__global__ __launch_bounds__(BLOCK) void compat_bits_kernel(const T* __restrict__ pairs, const int32_t* __restrict__ P, int n, int W, int bpc, T thr, T L,
                                                            uint64_t* __restrict__ adj, int32_t* __restrict__ degree, int64_t* __restrict__ degree2) {
    __shared__ T sx[3][C2_TILE], sy[3][C2_TILE];
    const int cloud = blockIdx.x / bpc, blk = blockIdx.x - cloud * bpc;
    const int Pc = min(max(P[cloud], 0), n);
    const int p = blk * BLOCK + (int)threadIdx.x;
    uint64_t* rows = adj + (size_t)cloud * n * W;
    if (p < n) degree2[(size_t)cloud * n + p] = 0;
    if (blk * BLOCK >= Pc) {                                // (block-uniform) no pair here: rows of zeros, one contiguous range
        const size_t first = (size_t)blk * BLOCK * W, count = (size_t)(min(n, (blk + 1) * BLOCK) - blk * BLOCK) * W;
        for (size_t e = threadIdx.x; e < count; e += BLOCK) rows[first + e] = 0;
        if (p < n) degree[(size_t)cloud * n + p] = 0;
        return;
    }
    const bool live = p < Pc;
    const T* base = pairs + (size_t)cloud * n * COMPAT_ROW;
    T r[COMPAT_ROW];
#pragma unroll
    for (int k = 0; k < COMPAT_ROW; ++k) r[k] = live ? base[(size_t)p * COMPAT_ROW + k] : T(0);
    int deg = 0;
    for (int q0 = 0; q0 < W * 64; q0 += C2_TILE) {
        const int len = min(max(Pc - q0, 0), C2_TILE);      // (block-uniform) live rows q of this tile
        const int words = min(C2_TW, W - q0 / 64);
        uint64_t word[C2_TW];
#pragma unroll
        for (int k = 0; k < C2_TW; ++k) word[k] = 0;
        if (len > 0) {
            __syncthreads();                                // the previous tile has been read
            for (int j = threadIdx.x; j < C2_TILE; j += BLOCK) {
                const bool in = j < len;                    // past the live rows: NaN, compatible with nothing
                const T* row = base + (size_t)(q0 + (in ? j : 0)) * COMPAT_ROW;
                sx[0][j] = in ? row[0] : c2_nan<T>(); sx[1][j] = in ? row[1] : c2_nan<T>(); sx[2][j] = in ? row[2] : c2_nan<T>();
                sy[0][j] = in ? row[3] : c2_nan<T>(); sy[1][j] = in ? row[4] : c2_nan<T>(); sy[2][j] = in ? row[5] : c2_nan<T>();
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < C2_TW; ++k) {
                if (k * 64 < len) {                         // (block-uniform)
                    uint32_t half[2] = {0u, 0u};
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
#pragma unroll 8
                        for (int jj = 0; jj < 32; ++jj) {
                            const int j = k * 64 + hh * 32 + jj;
                            const bool ok = compat_pair<T>(r[0], r[1], r[2], r[3], r[4], r[5], sx[0][j], sx[1][j], sx[2][j], sy[0][j], sy[1][j], sy[2][j], thr, L);
                            half[hh] |= compat2_bit(live, j < len, q0 + j == p, ok) ? (1u << jj) : 0u;
                        }
                    }
                    word[k] = ((uint64_t)half[1] << 32) | (uint64_t)half[0];
                    deg += compat2_popc(word[k]);
                }
            }
        }
        if (p < n) {
#pragma unroll
            for (int k = 0; k < C2_TW; ++k)
                if (k < words) rows[(size_t)p * W + q0 / 64 + k] = word[k];
        }
    }
    if (p < n) degree[(size_t)cloud * n + p] = deg;
}

__global__ __launch_bounds__(BLOCK) void compat_common_kernel(const uint64_t* __restrict__ adj, const int32_t* __restrict__ P, int n, int W, int ptiles, int qchunks,
                                                              unsigned long long* __restrict__ degree2) {
    __shared__ __align__(16) uint64_t sp[C2_WC][C2_LD], sq[C2_WC][C2_LD];
    const int qc = blockIdx.x % qchunks, rest = blockIdx.x / qchunks;
    const int pt = rest % ptiles, cloud = rest / ptiles;
    const int Pc = min(max(P[cloud], 0), n);
    const int p0 = pt * C2_TP, qbeg = qc * C2_QC;
    if (p0 >= Pc || qbeg >= Pc) return;                     // (block-uniform)
    const int qend = min(Pc, qbeg + C2_QC);
    const int Wl = compat2_words(Pc);                       // the words that can hold a bit (<= W)
    const uint64_t* rows = adj + (size_t)cloud * n * W;
    const int tp = (int)threadIdx.x >> 4, tq = (int)threadIdx.x & 15;
    unsigned long long tot[4] = {0ull, 0ull, 0ull, 0ull};
    for (int q0 = qbeg; q0 < qend; q0 += C2_TP) {
        int32_t cnt[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) cnt[i][j] = 0;
        for (int w0 = 0; w0 < Wl; w0 += C2_WC) {
            __syncthreads();                                // the previous chunk has been read
            for (int e = threadIdx.x; e < C2_TP * C2_WC; e += BLOCK) {
                const int rr = e / C2_WC, w = e - rr * C2_WC, gw = w0 + w;
                sp[w][rr] = (p0 + rr < n && gw < W) ? rows[(size_t)(p0 + rr) * W + gw] : 0;
                sq[w][rr] = (q0 + rr < n && gw < W) ? rows[(size_t)(q0 + rr) * W + gw] : 0;
            }
            __syncthreads();
            const int wl = min(C2_WC, Wl - w0);
#pragma unroll 2
            for (int w = 0; w < wl; ++w) {
                const ulonglong2* ap = reinterpret_cast<const ulonglong2*>(&sp[w][tp * 4]);
                const ulonglong2* bp = reinterpret_cast<const ulonglong2*>(&sq[w][tq * 4]);
                const ulonglong2 a01 = ap[0], a23 = ap[1], b01 = bp[0], b23 = bp[1];
                const uint64_t a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) cnt[i][j] += compat2_popc(a[i] & b[j]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {                       // S(p, q) = common where bit (p, q) is set
            const int p = p0 + tp * 4 + i;
            const uint64_t m = p < n ? rows[(size_t)p * W + (q0 >> 6)] : 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) tot[i] += ((m >> (tq * 4 + j)) & 1u) ? (unsigned long long)cnt[i][j] : 0ull;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned long long t = tot[i];
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) t += __shfl_xor(t, off);
        const int p = p0 + tp * 4 + i;
        if (tq == 0 && t && p < n) atomicAdd(degree2 + (size_t)cloud * n + p, t);
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void compat2_rank_kernel(const int64_t* __restrict__ degree2, const int32_t* __restrict__ P, int n, int bpc, int seeds,
                                                             int32_t* __restrict__ rank, T* __restrict__ score2, int32_t* __restrict__ seedpos) {
    __shared__ int64_t sd[C2_TILE];
    const int cloud = blockIdx.x / bpc, blk = blockIdx.x - cloud * bpc;
    const int Pc = min(max(P[cloud], 0), n);
    const int p = blk * BLOCK + (int)threadIdx.x;
    if (blk * BLOCK >= Pc) {                                // (block-uniform) no pair here: a rank past every keep
        if (p < n) { rank[(size_t)cloud * n + p] = 0x7fffffff; score2[(size_t)cloud * n + p] = T(0); }
        return;
    }
    const bool live = p < Pc;
    const int64_t* dc = degree2 + (size_t)cloud * n;
    const int64_t dp = live ? dc[p] : 0;
    int rk = 0;
    int64_t mx = 0;
    for (int q0 = 0; q0 < Pc; q0 += C2_TILE) {
        const int len = min(C2_TILE, Pc - q0);
        __syncthreads();
        for (int j = threadIdx.x; j < len; j += BLOCK) sd[j] = dc[q0 + j];
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < len; ++j) {
            const int64_t dq = sd[j];
            rk += compat2_before(dq, q0 + j, dp, p) ? 1 : 0;
            mx = dq > mx ? dq : mx;
        }
    }
    if (p < n) {
        rank[(size_t)cloud * n + p] = live ? rk : 0x7fffffff;
        score2[(size_t)cloud * n + p] = live ? compat2_score<T>(dp, mx) : T(0);
    }
    if (live && seedpos && rk < seeds) seedpos[(size_t)cloud * seeds + rk] = p;
}

template <typename T>
__global__ __launch_bounds__(WAVE) void compat2_seed_kernel(const T* __restrict__ pairs, const int32_t* __restrict__ P, const uint64_t* __restrict__ adj,
                                                            const int32_t* __restrict__ seedpos, int n, int W, int seeds, int members,
                                                            int32_t* __restrict__ member_list, T* __restrict__ poses) {
    __shared__ uint64_t list[C2_KMAX][WAVE];                // a lane's best keys, descending
    __shared__ int32_t smem[COMPAT2_MEMBERS_MAX];
    const int cloud = blockIdx.x / seeds, h = blockIdx.x - cloud * seeds;
    const int lane = (int)threadIdx.x;
    const int Pc = min(max(P[cloud], 0), n);
    const int K = members - 1;
    const uint64_t* rows = adj + (size_t)cloud * n * W;
    int count = 0;
    int32_t mine = -1;                                      // lane k ends up with member k
    int32_t s = h < Pc ? seedpos[(size_t)cloud * seeds + h] : -1;       // (wave-uniform)
    if (s >= 0 && s < Pc) {
        for (int k = 0; k < K; ++k) list[k][lane] = 0;
        const uint64_t* rs = rows + (size_t)s * W;
        const int Wl = compat2_words(Pc);
        for (int i = 0; i < Wl; ++i) {
            const uint64_t word = rs[i];                    // the bits of q = 64 i + lane
            if (word == 0) continue;                        // (wave-uniform)
            if ((word >> lane) & 1u) {
                const int q = i * 64 + lane;
                const int32_t S = compat2_common(rs, rows + (size_t)q * W, Wl);
                const uint64_t key = compat2_key(S, q);
                if (S > 0 && key > list[K - 1][lane]) {
                    int k = K - 1;
                    while (k > 0 && list[k - 1][lane] < key) { list[k][lane] = list[k - 1][lane]; --k; }
                    list[k][lane] = key;
                }
            }
        }
        if (lane == 0) mine = s;
        count = 1;
        int ptr = 0;
        for (int m = 0; m < K; ++m) {
            const uint64_t head = ptr < K ? list[ptr][lane] : 0;
            uint64_t best = head;
#pragma unroll
            for (int off = WAVE / 2; off > 0; off >>= 1) {
                const uint64_t o = __shfl_xor((unsigned long long)best, off);
                best = o > best ? o : best;
            }
            if (best == 0) break;                           // (wave-uniform) no candidate left
            if (head == best) ++ptr;                        // (the keys are distinct: one lane owns it)
            if (lane == count) mine = compat2_key_q(best);
            ++count;
        }
    }
    if (lane < members) {
        member_list[((size_t)cloud * seeds + h) * members + lane] = lane < count ? mine : -1;
        smem[lane] = lane < count ? mine : 0;
    }
    __syncthreads();
    if (lane == 0) {
        T pose[12];
        compat2_fit<T>(pairs + (size_t)cloud * n * RANSAC_ROW, smem, count, pose);
        T* out = poses + ((size_t)cloud * seeds + h) * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) out[k] = pose[k];
    }
}

inline int compat2_check(int dtype, int N, int n) {
    if (bad_dtype(dtype)) return DICP_ERR_DTYPE;
    if (N < 1 || n < 1 || n > COMPAT2_N_MAX) return DICP_ERR_SHAPE;
    const size_t W = (size_t)compat2_words(n);
    const size_t ptiles = ((size_t)n + C2_TP - 1) / C2_TP, qchunks = ((size_t)n + C2_QC - 1) / C2_QC;
    if ((size_t)N * ((size_t)(n + BLOCK - 1) / BLOCK) >= ((size_t)1 << 31) || (size_t)N * ptiles * qchunks >= ((size_t)1 << 31) ||
        (size_t)N * n * W >= ((size_t)1 << 40))
        return DICP_ERR_SHAPE;                              // the grids, the words
    return 0;
}

inline bool bad_seeds(int N, int seeds, int members) {
    return seeds < 1 || seeds > RANSAC_H_MAX || members < COMPAT2_MEMBERS_MIN || members > COMPAT2_MEMBERS_MAX || (size_t)N * seeds >= ((size_t)1 << 31);
}

}  // namespace

void dicp_compat2_geometry(int* rows, int* tile, int* words, int* chunk) {
    if (rows) *rows = C2_TP;
    if (tile) *tile = C2_TILE;
    if (words) *words = C2_WC;
    if (chunk) *chunk = C2_QC;
}

int dicp_compat2_bits(int dtype, const void* pairs, const int32_t* P, int N, int n, double threshold, double min_length, int64_t* adj, int32_t* degree,
                      int64_t* degree2, void* stream) {
    if (!pairs || !P || !adj || !degree || !degree2) return DICP_ERR_NULL;
    if (const int bad = compat2_check(dtype, N, n)) return bad;
    if (!(threshold > 0.0 && threshold < HUGE_VAL) || !(min_length >= 0.0 && min_length < HUGE_VAL)) return DICP_ERR_SHAPE;
    if (misaligned(pairs, elem_size(dtype)) || misaligned(P, 4) || misaligned(adj, 8) || misaligned(degree, 4) || misaligned(degree2, 8)) return DICP_ERR_ALIGN;
    const int bpc = (n + BLOCK - 1) / BLOCK;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        compat_bits_kernel<T><<<(unsigned)N * (unsigned)bpc, BLOCK, 0, (hipStream_t)stream>>>((const T*)pairs, P, n, compat2_words(n), bpc, compat_thr<T>(threshold),
                                                                                            compat_thr<T>(min_length), (uint64_t*)adj, degree, degree2);
    });
    return launch_status();
}

int dicp_compat2_common(const int64_t* adj, const int32_t* P, int N, int n, int64_t* degree2, void* stream) {
    if (!adj || !P || !degree2) return DICP_ERR_NULL;
    if (const int bad = compat2_check(DICP_F32, N, n)) return bad;
    if (misaligned(adj, 8) || misaligned(P, 4) || misaligned(degree2, 8)) return DICP_ERR_ALIGN;
    const int ptiles = (n + C2_TP - 1) / C2_TP, qchunks = (n + C2_QC - 1) / C2_QC;
    begin_launch();
    compat_common_kernel<<<(unsigned)N * (unsigned)ptiles * (unsigned)qchunks, BLOCK, 0, (hipStream_t)stream>>>((const uint64_t*)adj, P, n, compat2_words(n), ptiles,
                                                                                                             qchunks, (unsigned long long*)degree2);
    return launch_status();
}

int dicp_compat2_rank(int dtype, const int64_t* degree2, const int32_t* P, int N, int n, int seeds, int32_t* rank2, void* score2, int32_t* seedpos,
                      void* stream) {
    if (!degree2 || !P || !rank2 || !score2) return DICP_ERR_NULL;
    if (const int bad = compat2_check(dtype, N, n)) return bad;
    if (seeds < 0 || seeds > RANSAC_H_MAX || (seeds > 0) != (seedpos != nullptr) || (size_t)N * (size_t)seeds >= ((size_t)1 << 31)) return DICP_ERR_SHAPE;
    if (misaligned(degree2, 8) || misaligned(P, 4) || misaligned(rank2, 4) || misaligned(score2, elem_size(dtype)) || misaligned(seedpos, 4)) return DICP_ERR_ALIGN;
    const int bpc = (n + BLOCK - 1) / BLOCK;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        compat2_rank_kernel<T><<<(unsigned)N * (unsigned)bpc, BLOCK, 0, (hipStream_t)stream>>>(degree2, P, n, bpc, seeds, rank2, (T*)score2, seedpos);
    });
    return launch_status();
}

int dicp_compat2_seeds(int dtype, const void* pairs, const int32_t* P, const int64_t* adj, const int32_t* seedpos, int N, int n, int seeds, int members,
                       int32_t* member_list, void* poses, void* stream) {
    if (!pairs || !P || !adj || !seedpos || !member_list || !poses) return DICP_ERR_NULL;
    if (const int bad = compat2_check(dtype, N, n)) return bad;
    if (bad_seeds(N, seeds, members)) return DICP_ERR_SHAPE;
    const size_t ts = elem_size(dtype);
    if (misaligned(pairs, ts) || misaligned(poses, ts) || misaligned(P, 4) || misaligned(adj, 8) || misaligned(seedpos, 4) || misaligned(member_list, 4))
        return DICP_ERR_ALIGN;
    begin_launch();
    with_scalar(dtype, [&](auto t) {
        using T = decltype(t);
        compat2_seed_kernel<T><<<(unsigned)N * (unsigned)seeds, WAVE, 0, (hipStream_t)stream>>>((const T*)pairs, P, (const uint64_t*)adj, seedpos, n, compat2_words(n),
                                                                                              seeds, members, member_list, (T*)poses);
    });
    return launch_status();
}
