// rs_ochs.hip -- exact OCHS features (opponent-cluster hand strength: a hand's equity against each of up to 8 opponent ranges) of a flop, turn or river round, and the
// per-hole-pair EHS bin counts the preflop histograms are made of: the front end of gen_ochs (gen_abstraction/main.rs:161-330), with enumeration in place of the
// reference's sampled calc_equity.  Semantics: include/rustsolver_amd.h.  Everything before the last division is an integer, so results depend on the cards and the
// partition alone.
//   * k_ochs_round: one workgroup per board.  Per run-out the 1081 hole pairs are evaluated once and ordered by `score << 8 | cluster` in LDS; one exclusive prefix
//     count per cluster over that order (eight uint16 counters = two 64-bit words per position) gives, at the lower and upper bound of a pair's score, the hands of
//     every cluster that score lower or equal; the 46 + 46 pairs that hold one of its cards are taken off, cluster by cluster, in the same packed words.  Flop and turn
//     add (2 W + T, N) per (hole pair, cluster) into LDS; the last step divides, normalises and scatters the rows through hand_index.
//   * k_preflop_counts: a flop's LDS histogram as k_ehs_round_hist (rs_ehs.hip) builds it, then one atomicAdd per non-zero cell into the 1326 x n_bins table.
// The stages the sweeps share are one copy each in rs_ehs_dev.hpp: the board's decode, the run-out, the 1081 keys (k_ochs_round supplies `score << 8 | cluster`), the
// sort, the hole pair's number, and for k_preflop_counts the whole histogram of a board.  k_ochs_round's own: Packed8, the prefix scan, the packed card removal, the
// accumulators and the last step.
// Cards, suits and clusters only ever select under predicates (no private array indexed by one): the kernels carry no scratch (profiles/ochs.md).
#include <cstring>
#include <string>
#include <vector>

#include "rs_ehs_dev.hpp"

using namespace rs;

#define RS_HIP(call, what)                                   \
    do {                                                     \
        hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return rs::hip_fail(e_, what); \
    } while (0)

namespace rs {

constexpr uint32_t kHolePairs = 1326;  // C(52, 2)

// eight uint16 counters, clusters 0-3 in lo and 4-7 in hi.  No counter passes 1081, so sums and differences of such words never carry between counters.
struct Packed8 {
    uint64_t lo, hi;
};
__device__ __forceinline__ Packed8 one_of(uint32_t cluster) {   // one hand of `cluster`; nothing for RS_OCHS_NO_CLUSTER
    const uint64_t bit = 1ull << (16u * (cluster & 3u));
    return {cluster < 4u ? bit : 0ull, cluster >= 4u && cluster < (uint32_t)RS_OCHS_MAX_CLUSTERS ? bit : 0ull};
}
__device__ __forceinline__ uint32_t counter(const Packed8 &v, int k) { return (uint32_t)((k < 4 ? v.lo : v.hi) >> (16 * (k & 3))) & 0xffffu; }

// ---- the features ---------------------------------------------------------------------------------------------------------------------------------------
struct OchsSweep {
    HandIndexView view;
    const uint8_t *boards;   // [nb][pitch]
    uint32_t pitch;
    int32_t nb;              // 3, 4 or 5
    int32_t n_clusters;
    int32_t normalize;
    float *out;              // [size(1)][n_clusters]
    uint32_t *err;
    uint8_t pair_cluster[1328];   // [1326] by c1 (c1 - 1) / 2 + c0
};

constexpr uint32_t kOchsFixedWords = kEhsSortN + 1088u + 4u * kEhsSortN + 4u * (kSweepThreads / 64) + 1328u / 4u;
// LDS words of one workgroup: the sort buffer, the keys by pair number, the prefix counts, the waves' totals, the partition, the (2 W + T, N) accumulators
__host__ __device__ inline uint32_t ochs_lds_words(int nb, int n_clusters) {
    const uint32_t nf = 52u - (uint32_t)nb;
    return kOchsFixedWords + 2u * (uint32_t)n_clusters * (nf * (nf - 1) / 2);
}

__global__ __launch_bounds__(kSweepThreads, 4) void k_ochs_round(const OchsSweep a) {
    extern __shared__ uint32_t ochs_lds[];
    uint32_t *sorted = ochs_lds;                                                 // [kEhsSortN] score << 8 | cluster, ascending
    uint32_t *sc = sorted + kEhsSortN;                                            // [1088] the key of pair p
    Packed8 *prefix = reinterpret_cast<Packed8 *>(sc + 1088);                     // [kEhsSortN] hands of each cluster in front of a position of the order
    Packed8 *wave_total = prefix + kEhsSortN;                                     // [16]
    uint8_t *pc = reinterpret_cast<uint8_t *>(wave_total + kSweepThreads / 64);    // [1328]
    uint32_t *acc = reinterpret_cast<uint32_t *>(pc + 1328);                      // [n_clusters][2][n_hp]: 2 W + T, N
    const int nb = a.nb, ncl = a.n_clusters;
    const uint32_t nf = 52u - (uint32_t)nb, n_hp = nf * (nf - 1) / 2;
    const uint32_t n_ro = nb == 3 ? 1176u : (nb == 4 ? 48u : 1u);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;

    uint32_t bc[5], bm[4] = {0, 0, 0, 0};
    uint64_t board;
    __builtin_assume(a.boards != nullptr);   // the host always lists the boards (class_boards): the numbered decode drops out of this kernel
    if (!sweep_board(a.boards, a.pitch, nb, bc, board, bm)) {   // uniform over the workgroup: reported, nothing written
        if (tid == 0) atomicOr(a.err, 1u);
        return;
    }
    const uint64_t free0 = kDeck & ~board;   // nf cards

    for (uint32_t i = tid; i < 1328u; i += kSweepThreads) pc[i] = a.pair_cluster[i];
    for (uint32_t i = tid; i < 2u * (uint32_t)ncl * n_hp; i += kSweepThreads) acc[i] = 0;
    __syncthreads();

    for (uint32_t ro = 0; ro < n_ro; ++ro) {
        uint32_t b5[4] = {bm[0], bm[1], bm[2], bm[3]};
        uint64_t free5;   // 47 cards
        run_out(nb, free0, ro, b5, free5);
        fill_keys(b5, free5, sc, sorted, tid, [pc](uint32_t score, uint32_t ci, uint32_t cj) {
            const uint32_t hi = ci > cj ? ci : cj, lo = ci > cj ? cj : ci;
            return score << 8 | pc[hi * (hi - 1) / 2 + lo];   // a score has 24 bits
        });
        sort_keys(sorted, tid);

        // exclusive prefix counts: a thread sums its two positions, the wave scans, the waves' totals carry over
        {
            const Packed8 v0 = one_of(sorted[2 * tid] & 255u), v1 = one_of(sorted[2 * tid + 1] & 255u);
            uint64_t lo = v0.lo + v1.lo, hi = v0.hi + v1.hi;
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint64_t xl = __shfl_up((unsigned long long)lo, d), xh = __shfl_up((unsigned long long)hi, d);
                if (lane >= d) {
                    lo += xl;
                    hi += xh;
                }
            }
            if (lane == 63) wave_total[wave] = {lo, hi};
            __syncthreads();
            for (uint32_t w = 0; w < wave; ++w) {
                lo += wave_total[w].lo;
                hi += wave_total[w].hi;
            }
            lo -= v0.lo + v1.lo;
            hi -= v0.hi + v1.hi;
            prefix[2 * tid] = {lo, hi};
            prefix[2 * tid + 1] = {lo + v0.lo, hi + v0.hi};
        }
        __syncthreads();

        for (uint32_t p = tid; p < kEhsPairs; p += kSweepThreads) {
            uint32_t i, j;
            pair_of<47>(p, i, j);
            const uint32_t key = sc[p], s = key >> 8;
            // hands that score lower / no higher among all 1081 pairs
            const uint32_t k_lo = s << 8, k_hi = (s + 1u) << 8;
            uint32_t lb = 0, ub = 0;
#pragma unroll
            for (uint32_t step = kEhsSortN / 2; step; step >>= 1) {
                if (sorted[lb + step - 1] < k_lo) lb += step;
                if (sorted[ub + step - 1] < k_hi) ub += step;
            }
            // ... and, cluster by cluster, among the 46 pairs that hold its first card and the 46 that hold its second (it stands in both lists)
            Packed8 below = {0, 0}, equal = {0, 0}, held = {0, 0};
            for (uint32_t d = 1; d <= 23; ++d) {
                const uint32_t q[4] = {sc[i * 23 + d - 1], sc[((i + 47 - d) % 47) * 23 + d - 1], sc[j * 23 + d - 1], sc[((j + 47 - d) % 47) * 23 + d - 1]};
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const Packed8 one = one_of(q[x] & 255u);
                    const uint32_t sq = q[x] >> 8;
                    held.lo += one.lo;
                    held.hi += one.hi;
                    below.lo += sq < s ? one.lo : 0ull;
                    below.hi += sq < s ? one.hi : 0ull;
                    equal.lo += sq == s ? one.lo : 0ull;
                    equal.hi += sq == s ? one.hi : 0ull;
                }
            }
            const Packed8 self = one_of(key & 255u), at_lb = prefix[lb], at_ub = prefix[ub], total = prefix[kEhsPairs];
            // the pair itself was taken off twice: put back once, in its own cluster, which leaves it out of T and N
            const Packed8 w = {at_lb.lo - below.lo, at_lb.hi - below.hi};
            const Packed8 t = {at_ub.lo - at_lb.lo + self.lo - equal.lo, at_ub.hi - at_lb.hi + self.hi - equal.hi};
            const Packed8 n = {total.lo + self.lo - held.lo, total.hi + self.hi - held.hi};
            const Packed8 k2 = {2ull * w.lo + t.lo, 2ull * w.hi + t.hi};   // at most 2 * 990 per counter
            uint32_t *cell = acc + hole_pair_number(free0, free5, i, j);   // one thread per hole pair and run-out, so plain adds
#pragma unroll
            for (int k = 0; k < RS_OCHS_MAX_CLUSTERS; ++k)
                if (k < ncl) {
                    cell[(2 * k) * n_hp] += counter(k2, k);
                    cell[(2 * k + 1) * n_hp] += counter(n, k);
                }
        }
        __syncthreads();
    }

    // divide, normalise and scatter through the indexer; the card bytes of a hand stand in LDS (the sort buffer is free now) so that hand_index reads no private array
    uint8_t *hand = reinterpret_cast<uint8_t *>(sorted) + tid * 8u;
    for (uint32_t hp = tid; hp < n_hp; hp += kSweepThreads) {
        uint32_t lo, hi;
        pair_positions(hp, lo, hi);
        hand[0] = (uint8_t)nth_bit(free0, lo);
        hand[1] = (uint8_t)nth_bit(free0, hi);
#pragma unroll
        for (int i = 0; i < 5; ++i)
            if (i < nb) hand[2 + i] = (uint8_t)bc[i];
        const uint64_t row = hand_index(a.view, 1, hand);
        float e[RS_OCHS_MAX_CLUSTERS], sum = 0.0f;
#pragma unroll
        for (int k = 0; k < RS_OCHS_MAX_CLUSTERS; ++k) {
            e[k] = 0.0f;
            if (k < ncl) {
                const uint32_t k2 = acc[(2 * k) * n_hp + hp], n = acc[(2 * k + 1) * n_hp + hp];
                if (n) e[k] = (float)((double)k2 / (double)(2u * n));
                sum += e[k];
            }
        }
        float *dst = a.out + row * (uint64_t)ncl;
#pragma unroll
        for (int k = 0; k < RS_OCHS_MAX_CLUSTERS; ++k)
            if (k < ncl) dst[k] = a.normalize ? (sum != 0.0f ? e[k] / sum : 0.0f) : e[k];
    }
}

// ---- the preflop counts ---------------------------------------------------------------------------------------------------------------------------------
struct PreflopSweep {
    EhsBins bins;
    const uint8_t *boards;   // [3][pitch], or nullptr: flop number blockIdx.x of all 22 100
    uint32_t pitch;
    uint32_t *counts;        // [1326][n_bins]
    uint32_t *err;
};

__global__ __launch_bounds__(kSweepThreads, 8) void k_preflop_counts(const PreflopSweep a) {
    extern __shared__ uint32_t ochs_lds[];
    const HistLds l = carve_hist_lds(ochs_lds);
    const int n_bins = a.bins.n_bins;
    const uint32_t tid = threadIdx.x;

    uint32_t bc[5], bm[4] = {0, 0, 0, 0};
    uint64_t board;
    if (!sweep_board(a.boards, a.pitch, 3, bc, board, bm)) {
        if (tid == 0) atomicOr(a.err, 1u);
        return;
    }
    const uint64_t free0 = kDeck & ~board;   // 49 cards
    board_histogram(3, a.bins, free0, bm, l, tid);

    // the board's non-zero cells into the table, by the pair's card numbers; integer adds, so their order is free
    for (uint32_t hp = tid; hp < 1176u; hp += kSweepThreads) {
        uint32_t lo, hi;
        pair_positions(hp, lo, hi);
        const uint32_t c0 = nth_bit(free0, lo), c1 = nth_bit(free0, hi);   // c0 < c1
        uint32_t *dst = a.counts + (size_t)(c1 * (c1 - 1) / 2 + c0) * (uint32_t)n_bins;
        for (int k = 0; k < n_bins; ++k) {
            const uint32_t count = hist_count(l.hist, hp * (uint32_t)n_bins + (uint32_t)k);
            if (count) atomicAdd(&dst[k], count);
        }
    }
}

// dynamic LDS beyond what a launch gets unasked
int grant_lds(const void *kernel, size_t lds, const char *who) {
    if (lds <= 64 * 1024) return RS_OK;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e == hipSuccess) return RS_OK;
    (void)hipGetLastError();
    return fail(RS_ERR_UNSUPPORTED, std::string(who) + ": the device grants no workgroup " + std::to_string(lds) + " bytes of LDS (" + hipGetErrorString(e) + ")");
}

// one representative board per suit-isomorphism class of the nb-card boards, as SoA rows [nb][pitch]
int class_boards(int nb, std::vector<uint8_t> *rows, uint32_t *n, uint32_t *pitch) {
    const uint8_t cpr[1] = {(uint8_t)nb};
    rs_hand_indexer *ix = nullptr;
    if (int rc = rs_hand_indexer_create(1, cpr, &ix)) return rc;
    const uint64_t size = rs_hand_indexer_size(ix, 0);
    if (size != (nb == 3 ? 1755u : nb == 4 ? 16432u : 134459u)) {
        rs_hand_indexer_destroy(ix);
        return fail(RS_ERR_INVALID, "rs_ochs_round_features: the board indexer has " + std::to_string(size) + " classes");
    }
    std::vector<uint64_t> idx(size);
    for (uint64_t i = 0; i < size; ++i) idx[i] = i;
    std::vector<uint8_t> aos(size * nb);
    const int rc = rs_hand_unindex(ix, 0, idx.data(), size, aos.data());
    rs_hand_indexer_destroy(ix);
    if (rc) return rc;
    *n = uint32_t(size);
    *pitch = uint32_t(round_up(size, kLanePad));
    rows->assign(size_t(nb) * *pitch, 0);
    for (uint64_t i = 0; i < size; ++i)
        for (int c = 0; c < nb; ++c) (*rows)[size_t(c) * *pitch + i] = aos[i * nb + c];
    return RS_OK;
}

}  // namespace rs

extern "C" {

int rs_ochs_round_features(rs_table *t, rs_hand_indexer *ix, const uint8_t *pair_cluster, int n_clusters, int normalize, const uint8_t *d_boards, uint32_t n_boards,
                           float *d_out) {
    if (!t || !ix || !pair_cluster) return fail(RS_ERR_INVALID, "rs_ochs_round_features: NULL argument");
    const int nc = rs_hand_indexer_n_cards(ix, 1);
    if (rs_hand_indexer_rounds(ix) != 2 || rs_hand_indexer_n_cards(ix, 0) != 2 || (nc != 5 && nc != 6 && nc != 7))
        return fail(RS_ERR_INVALID, "rs_ochs_round_features: the indexer must be hand_indexer_s::init(2, [2, 3]) (flop), (2, [2, 4]) (turn) or (2, [2, 5]) (river)");
    if (n_clusters < 1 || n_clusters > RS_OCHS_MAX_CLUSTERS) return fail(RS_ERR_INVALID, "rs_ochs_round_features: n_clusters must be 1..RS_OCHS_MAX_CLUSTERS");
    for (uint32_t i = 0; i < kHolePairs; ++i)
        if (pair_cluster[i] >= n_clusters && pair_cluster[i] != RS_OCHS_NO_CLUSTER)
            return fail(RS_ERR_INVALID, "rs_ochs_round_features: pair_cluster[" + std::to_string(i) + "] = " + std::to_string(pair_cluster[i]) + " is neither a cluster below n_clusters nor RS_OCHS_NO_CLUSTER");
    const int nb = nc - 2;
    if ((!d_boards || n_boards) && !d_out) return fail(RS_ERR_INVALID, "rs_ochs_round_features: NULL output");
    if (d_boards && n_boards == 0) return RS_OK;
    if (int rc_ = rs::table_settle(t, false)) return rc_;
    RS_HIP(hipSetDevice(t->device), "hipSetDevice");
    OchsSweep a;
    std::memset(&a, 0, sizeof(a));
    if (int rc = hand_indexer_view_on(ix, t->device, t->stream, &a.view)) return rc;
    const size_t lds = size_t(ochs_lds_words(nb, n_clusters)) * sizeof(uint32_t);
    if (int rc = grant_lds(reinterpret_cast<const void *>(k_ochs_round), lds, "rs_ochs_round_features")) return rc;
    DevBuf<uint8_t> d_classes;   // the whole round: one board per suit-isomorphism class reaches every canonical row
    a.boards = d_boards;
    a.pitch = uint32_t(round_up(n_boards, kLanePad));
    if (!d_boards) {
        std::vector<uint8_t> rows;
        if (int rc = class_boards(nb, &rows, &n_boards, &a.pitch)) return rc;
        RS_HIP(d_classes.alloc(rows.size()), "rs_ochs_round_features: the round's boards");
        RS_HIP(hipMemcpyAsync(d_classes, rows.data(), rows.size(), hipMemcpyHostToDevice, t->stream), "rs_ochs_round_features");
        RS_HIP(hipStreamSynchronize(t->stream), "rs_ochs_round_features");   // `rows` leaves scope
        a.boards = d_classes;
    }
    std::memset(a.pair_cluster, RS_OCHS_NO_CLUSTER, sizeof(a.pair_cluster));
    std::memcpy(a.pair_cluster, pair_cluster, kHolePairs);
    a.nb = nb;
    a.n_clusters = n_clusters;
    a.normalize = normalize;
    a.out = d_out;
    return launch_checked(t, "rs_ochs_round_features", "k_ochs_round", "a board", [&](uint32_t *d_err) {
        a.err = d_err;
        hipLaunchKernelGGL(k_ochs_round, dim3(n_boards), dim3(kSweepThreads), lds, t->stream, a);
    });
}

int rs_ehs_preflop_counts(rs_table *t, int n_bins, const uint8_t *d_boards, uint32_t n_boards, uint32_t *d_counts) {
    if (!t) return fail(RS_ERR_INVALID, "rs_ehs_preflop_counts: NULL table");
    if (n_bins < 1 || n_bins > RS_EHS_MAX_BINS) return fail(RS_ERR_INVALID, "rs_ehs_preflop_counts: n_bins must be 1..RS_EHS_MAX_BINS");
    if (!d_boards) n_boards = 22100u;
    if (!d_counts) return fail(RS_ERR_INVALID, "rs_ehs_preflop_counts: NULL output");
    if (int rc_ = rs::table_settle(t, false)) return rc_;
    RS_HIP(hipSetDevice(t->device), "hipSetDevice");
    RS_HIP(hipMemsetAsync(d_counts, 0, size_t(kHolePairs) * n_bins * sizeof(uint32_t), t->stream), "rs_ehs_preflop_counts");
    if (n_boards == 0) {
        RS_HIP(hipStreamSynchronize(t->stream), "rs_ehs_preflop_counts");
        return RS_OK;
    }
    PreflopSweep a;
    std::memset(&a, 0, sizeof(a));
    ehs_thresholds(n_bins, a.bins.thr);
    a.bins.n_bins = n_bins;
    a.boards = d_boards;
    a.pitch = uint32_t(round_up(n_boards, kLanePad));
    a.counts = d_counts;
    const size_t lds = size_t(ehs_sweep_lds_words(3, n_bins)) * sizeof(uint32_t);
    if (int rc = grant_lds(reinterpret_cast<const void *>(k_preflop_counts), lds, "rs_ehs_preflop_counts")) return rc;
    return launch_checked(t, "rs_ehs_preflop_counts", "k_preflop_counts", "a board", [&](uint32_t *d_err) {
        a.err = d_err;
        hipLaunchKernelGGL(k_preflop_counts, dim3(n_boards), dim3(kSweepThreads), lds, t->stream, a);
    });
}

}  // extern "C"
