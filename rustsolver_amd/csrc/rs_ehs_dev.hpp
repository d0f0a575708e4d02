// rs_ehs_dev.hpp -- what the enumeration kernels of rs_ehs.hip (exact EHS, the EHS histograms) and rs_ochs.hip (OCHS features, the preflop counts) share.  Numbering:
// the cards and pairs, get_bin over staged thresholds.  The stages of a board's sweep, one copy each: the decode of a listed or numbered board (sweep_board), a run-out's
// cards (run_out), the 1081 pairs evaluated into keys (fill_keys), their sort (sort_keys), a hole pair's number on the board (hole_pair_number, pair_positions), and the
// whole uint16 histogram of a board (board_histogram, hist_count) that k_ehs_round_hist and k_preflop_counts end differently.  Host: the thresholds, the histogram's LDS
// size, and a launch with an error word (launch_checked; grant_lds and class_boards are defined in rs_ochs.hip).  Cards and suits only ever select under predicates (no array
// indexed by a card), so nothing here costs a kernel scratch.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "rs_hand_index.hpp"
#include "rs_internal.hpp"
#include "rs_eval.hpp"

namespace rs {

constexpr uint32_t kEhsOpp = 990;      // C(45, 2) opponent hands of a 7-card hand
constexpr uint32_t kEhsPairs = 1081;   // C(47, 2) hole pairs of a 5-card board
constexpr uint32_t kEhsSortN = 2048;   // the bitonic network's width
constexpr uint64_t kDeck = (1ull << 52) - 1;
constexpr uint32_t kNoKey = 0xffffffffu;   // padding of the sort: behind every score, in no cluster
// The workgroup of the three sweep kernels, half the sort width: sort_keys and the shared loops stride by it, and a thread of k_ochs_round owns two positions of the order
// when the prefix counts are built.  LDS allows the histogram kernels two workgroups per CU at 20-30 bins, so a workgroup brings 16 waves (profiles/ehs.md)
constexpr int kSweepThreads = 1024;
static_assert(2 * kSweepThreads == kEhsSortN, "a thread of k_ochs_round owns two positions of the sorted order");

// thr[b], b = 1 .. n_bins - 1: get_bin's thresholds as its loop accumulates them (thr[0] is never read).  Non-decreasing in b.
struct EhsBins {
    float thr[RS_EHS_MAX_BINS];
    int32_t n_bins;
};

// position of the n-th (from 0) set bit of m; n < popcount(m)
__device__ __forceinline__ uint32_t nth_bit(uint64_t m, uint32_t n) {
    uint32_t w = (uint32_t)m, pos = 0, c = (uint32_t)__popc(w);
    if (n >= c) {
        n -= c;
        w = (uint32_t)(m >> 32);
        pos = 32;
    }
#pragma unroll
    for (int sh = 16; sh >= 1; sh >>= 1) {
        const uint32_t lo = w & ((1u << sh) - 1u);
        c = (uint32_t)__popc(lo);
        if (n >= c) {
            n -= c;
            w >>= sh;
            pos += (uint32_t)sh;
        } else w = lo;
    }
    return pos;
}

// Unordered pairs of M elements, M odd, numbered 0 .. M (M - 1) / 2 - 1: pair p = (a, (a + d) mod M) with a = p / H, d = p % H + 1, H = (M - 1) / 2 -- every
// pair has exactly one circular distance in 1 .. H.  The pairs that hold element i are i * H + d - 1 and ((i - d) mod M) * H + d - 1, d = 1 .. H.
template <uint32_t M>
__device__ __forceinline__ void pair_of(uint32_t p, uint32_t &i, uint32_t &j) {
    constexpr uint32_t H = (M - 1) / 2;
    i = p / H;
    j = (i + p % H + 1) % M;
}

// get_bin over the staged thresholds: the largest b with v > thr[b], else 0 (thr is non-decreasing, so the predicate is monotone in b)
__device__ __forceinline__ uint32_t ehs_bin_of(const float *thr, int n_bins, float v) {
    int b = 0;
#pragma unroll
    for (int step = RS_EHS_MAX_BINS / 2; step; step >>= 1) {
        const int c = b + step;
        if (c < n_bins && v > thr[c]) b = c;
    }
    return (uint32_t)b;
}

// the board with colexicographic number idx among the C(52, nb) boards: idx = C(c0, 1) + C(c1, 2) + C(c2, 3) (+ C(c3, 4)), c0 < c1 < c2 (< c3)
__device__ __forceinline__ uint32_t colex_digit(uint32_t &idx, int k) {
    uint32_t x = 51;
    while (hi_choose(x, k) > idx) --x;
    idx -= (uint32_t)hi_choose(x, k);
    return x;
}

// board number `at` of a list boards[nb][pitch], nb <= 5: its cards as listed, its card mask and its suit masks.  false: it repeats a card or holds a byte that is
// no card (such a byte never becomes a shift count or an index)
__device__ __forceinline__ bool listed_board(const uint8_t *__restrict__ boards, uint32_t pitch, int nb, uint32_t at, uint32_t (&bc)[5], uint64_t &mask, uint32_t (&suits)[4]) {
    bool ok = true;
    mask = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        bc[i] = 0;
        if (i < nb) {
            bc[i] = boards[(size_t)i * pitch + at];
            ok = ok && bc[i] < 52u;
            mask |= 1ull << (bc[i] & 63u);
        }
    }
    if (!ok || __popcll(mask) != nb) return false;
#pragma unroll
    for (int i = 0; i < 5; ++i)
        if (i < nb) add_card(suits, bc[i]);
    return true;
}

// the board of workgroup blockIdx.x: of the list, or with no list the board with that number among all C(52, nb), nb = 3 or 4.  Its cards are added to `suits`
// (the caller's zeros); false as listed_board
__device__ __forceinline__ bool sweep_board(const uint8_t *__restrict__ boards, uint32_t pitch, int nb, uint32_t (&bc)[5], uint64_t &mask, uint32_t (&suits)[4]) {
    if (boards) return listed_board(boards, pitch, nb, blockIdx.x, bc, mask, suits);
    uint32_t idx = blockIdx.x;
    bc[4] = 0;
    bc[3] = nb == 4 ? colex_digit(idx, 4) : 0u;
    bc[2] = colex_digit(idx, 3);
    bc[1] = colex_digit(idx, 2);
    bc[0] = idx;
    mask = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < nb) {
            mask |= 1ull << bc[i];
            add_card(suits, bc[i]);
        }
    return true;
}

// the 5-card board and its free cards after run-out `ro` of a board of nb cards (nb = 5: the board itself)
__device__ __forceinline__ void run_out(int nb, uint64_t free0, uint32_t ro, uint32_t (&b5)[4], uint64_t &free5) {
    free5 = free0;
    if (nb == 4) {
        const uint32_t c = nth_bit(free0, ro);
        add_card(b5, c);
        free5 &= ~(1ull << c);
    } else if (nb == 3) {
        uint32_t i, j;
        pair_of<49>(ro, i, j);
        const uint32_t ci = nth_bit(free0, i), cj = nth_bit(free0, j);
        add_card(b5, ci);
        add_card(b5, cj);
        free5 &= ~(1ull << ci | 1ull << cj);
    }
}

// the 1081 hole pairs of a 5-card board into sc[p] and sorted[p], padding behind: key(score, ci, cj) of the pair of cards ci, cj.  Ends on a barrier
template <class Key>
__device__ __forceinline__ void fill_keys(const uint32_t (&b5)[4], uint64_t free5, uint32_t *sc, uint32_t *sorted, uint32_t tid, Key key) {
    for (uint32_t p = tid; p < kEhsSortN; p += kSweepThreads) {
        uint32_t k = kNoKey;
        if (p < kEhsPairs) {
            uint32_t i, j;
            pair_of<47>(p, i, j);
            const uint32_t ci = nth_bit(free5, i), cj = nth_bit(free5, j);
            uint32_t m[4] = {b5[0], b5[1], b5[2], b5[3]};
            add_card(m, ci);
            add_card(m, cj);
            k = key(evaluate_suits(m), ci, cj);
            sc[p] = k;
        }
        sorted[p] = k;
    }
    __syncthreads();
}

// ascending bitonic sort of sorted[kEhsSortN] by the whole workgroup; ends on a barrier
__device__ __forceinline__ void sort_keys(uint32_t *sorted, uint32_t tid) {
    for (uint32_t k = 2; k <= kEhsSortN; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < kEhsSortN / 2; t += kSweepThreads) {
                const uint32_t lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), hi = lo | j;
                const uint32_t x = sorted[lo], y = sorted[hi];
                if ((x > y) == ((lo & k) == 0)) {
                    sorted[lo] = y;
                    sorted[hi] = x;
                }
            }
            __syncthreads();
        }
}

// the number, among the pairs of the board's free cards free0, of the hole pair at positions (i, j) of the run-out's free cards free5
__device__ __forceinline__ uint32_t hole_pair_number(uint64_t free0, uint64_t free5, uint32_t i, uint32_t j) {
    const uint32_t ci = nth_bit(free5, i), cj = nth_bit(free5, j);
    const uint32_t pi = (uint32_t)__popcll(free0 & ((1ull << ci) - 1)), pj = (uint32_t)__popcll(free0 & ((1ull << cj) - 1));
    const uint32_t hi = pi > pj ? pi : pj, lo = pi > pj ? pj : pi;
    return hi * (hi - 1) / 2 + lo;
}

// ... and back: hole pair number hp = hi (hi - 1) / 2 + lo over positions lo < hi
__device__ __forceinline__ void pair_positions(uint32_t hp, uint32_t &lo, uint32_t &hi) {
    hi = (uint32_t)((1.0f + sqrtf(1.0f + 8.0f * (float)hp)) * 0.5f);
    while (hi * (hi - 1) / 2 > hp) --hi;
    while ((hi + 1) * hi / 2 <= hp) ++hi;
    lo = hp - hi * (hi - 1) / 2;
}

// ---- the histogram of a board -------------------------------------------------------------------------------------------------------------------------------
// LDS words of one workgroup: the sort buffer, the scores by pair number, the thresholds, the histogram (two uint16 counters per word)
__host__ __device__ inline uint32_t ehs_sweep_lds_words(int nb, int n_bins) {
    const uint32_t nf = 52u - (uint32_t)nb, n_hp = nf * (nf - 1) / 2;
    return kEhsSortN + 1088u + (uint32_t)RS_EHS_MAX_BINS + (n_hp * (uint32_t)n_bins + 1u) / 2u;
}

struct HistLds {
    uint32_t *sorted;   // [kEhsSortN]
    uint32_t *sc;       // [1088] score of pair p
    float *thr;         // [RS_EHS_MAX_BINS]
    uint32_t *hist;     // [n_hp][n_bins] uint16, two to a word
};
__device__ __forceinline__ HistLds carve_hist_lds(uint32_t *lds) {
    return {lds, lds + kEhsSortN, reinterpret_cast<float *>(lds + kEhsSortN + 1088), lds + kEhsSortN + 1088 + RS_EHS_MAX_BINS};
}

__device__ __forceinline__ uint32_t hist_count(const uint32_t *hist, uint32_t cell) { return (hist[cell >> 1] >> (16u * (cell & 1u))) & 0xffffu; }

// The (hole pair, bin) counts of one board of nb = 3 or 4 cards over all its run-outs, by the whole workgroup, left in l.hist.  Per run-out the 1081 hole pairs are
// evaluated once and ordered by score, and each pair's counts come from the rank order with card removal, the way the best-response leaves count (rs_br.hip)
__device__ __forceinline__ void board_histogram(int nb, const EhsBins &bins, uint64_t free0, const uint32_t (&bm)[4], const HistLds l, uint32_t tid) {
    const int n_bins = bins.n_bins;
    const uint32_t nf = 52u - (uint32_t)nb, n_hp = nf * (nf - 1) / 2;
    const uint32_t n_ro = nb == 3 ? 1176u : 48u;   // run-outs of the board
    for (uint32_t i = tid; i < (uint32_t)RS_EHS_MAX_BINS; i += kSweepThreads) l.thr[i] = bins.thr[i];
    for (uint32_t i = tid; i < (n_hp * (uint32_t)n_bins + 1u) / 2u; i += kSweepThreads) l.hist[i] = 0;
    __syncthreads();

    for (uint32_t ro = 0; ro < n_ro; ++ro) {
        uint32_t b5[4] = {bm[0], bm[1], bm[2], bm[3]};
        uint64_t free5;   // 47 cards
        run_out(nb == 4 ? 4 : 3, free0, ro, b5, free5);
        fill_keys(b5, free5, l.sc, l.sorted, tid, [](uint32_t score, uint32_t, uint32_t) { return score; });
        sort_keys(l.sorted, tid);
        for (uint32_t p = tid; p < kEhsPairs; p += kSweepThreads) {
            uint32_t i, j;
            pair_of<47>(p, i, j);
            const uint32_t s = l.sc[p];
            // scores below and equal among all 1081 pairs (the pair itself is one of the equal ones)
            uint32_t lb = 0, ub = 0;
#pragma unroll
            for (uint32_t step = kEhsSortN / 2; step; step >>= 1) {
                if (l.sorted[lb + step - 1] < s) lb += step;
                if (l.sorted[ub + step - 1] <= s) ub += step;
            }
            // ... and among the 46 pairs that hold its first card and the 46 that hold its second (it stands in both lists)
            uint32_t below = 0, equal = 0;
            for (uint32_t d = 1; d <= 23; ++d) {
                const uint32_t q0 = l.sc[i * 23 + d - 1], q1 = l.sc[((i + 47 - d) % 47) * 23 + d - 1];
                const uint32_t q2 = l.sc[j * 23 + d - 1], q3 = l.sc[((j + 47 - d) % 47) * 23 + d - 1];
                below += (q0 < s) + (q1 < s) + (q2 < s) + (q3 < s);
                equal += (q0 == s) + (q1 == s) + (q2 == s) + (q3 == s);
            }
            const uint32_t w = lb - below, t = (ub - lb) - equal + 1u;   // over the 990 hands that share no card with it
            const float v = (float)((double)(2u * w + t) / (double)(2u * kEhsOpp));
            const uint32_t cell = hole_pair_number(free0, free5, i, j) * (uint32_t)n_bins + ehs_bin_of(l.thr, n_bins, v);
            atomicAdd(&l.hist[cell >> 1], 1u << (16u * (cell & 1u)));   // a counter never passes n_ro <= 1176: no carry into its neighbour
        }
        __syncthreads();
    }
}

// ---- the host ---------------------------------------------------------------------------------------------------------------------------------------------------
// get_bin's thresholds (gen_abstraction/main.rs:58-70), accumulated in f32 exactly as its loop does
inline void ehs_thresholds(int n_bins, float *thr) {
    const float interval = 1.0f / (float)n_bins;
    float threshold = 1.0f - interval;
    thr[0] = 0.0f;
    for (int bin = n_bins - 1; bin > 0; --bin) {
        thr[bin] = threshold;
        threshold -= interval;
    }
}

// dynamic LDS beyond what a launch gets unasked (rs_ochs.hip)
int grant_lds(const void *kernel, size_t lds, const char *who);
// one representative board per suit-isomorphism class of the nb-card boards, as SoA rows [nb][pitch] (rs_ochs.hip)
int class_boards(int nb, std::vector<uint8_t> *rows, uint32_t *n, uint32_t *pitch);

// A launch with an error word: the word allocated and zeroed on the table's stream, launch(word) to enqueue `kernel`, then the launch's own error and the word read
// back.  A set word is RS_ERR_INVALID: `what` repeats a card or holds a byte that is no card.  With `word` the word goes there instead and the caller words the refusal
template <class Launch>
int launch_checked(rs_table *t, const char *who, const char *kernel, const char *what, Launch launch, uint32_t *word = nullptr) {
    DevBuf<uint32_t> d_err;
    hipError_t e = d_err.alloc(1);
    if (e != hipSuccess) return hip_fail(e, (std::string(who) + ": error word").c_str());
    e = hipMemsetAsync(d_err, 0, sizeof(uint32_t), t->stream);
    if (e != hipSuccess) return hip_fail(e, who);
    launch(d_err.get());
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, kernel);
    uint32_t err = 0;
    e = hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) return hip_fail(e, who);
    if (word) {
        *word = err;
        return RS_OK;
    }
    if (err) return fail(RS_ERR_INVALID, std::string(who) + ": " + what + " repeats a card or holds a byte that is not a card (0..51); nothing was written for it");
    return RS_OK;
}

}  // namespace rs
