// rs_ehs_dev.hpp -- what the enumeration kernels of rs_ehs.hip (exact EHS, the EHS histograms) and rs_ochs.hip (OCHS features, the preflop counts) share: the card
// and pair numbering, get_bin over staged thresholds, the decode of a board, and the host's thresholds and error-word read-back.  Cards and suits only ever select
// under predicates (no array indexed by a card), so nothing here costs a kernel scratch.
#pragma once

#include <cstdint>
#include <string>

#include "rs_hand_index.hpp"
#include "rs_internal.hpp"
#include "rs_eval.hpp"

namespace rs {

constexpr uint32_t kEhsOpp = 990;      // C(45, 2) opponent hands of a 7-card hand
constexpr uint32_t kEhsPairs = 1081;   // C(47, 2) hole pairs of a 5-card board
constexpr uint32_t kEhsSortN = 2048;   // the bitonic network's width
constexpr uint64_t kDeck = (1ull << 52) - 1;

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

// the kernels' error word, read back by the call
inline int ehs_read_err(rs_table *t, const uint32_t *d_err, const char *who, const char *what) {
    uint32_t err = 0;
    hipError_t e = hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) return hip_fail(e, who);
    if (err) return fail(RS_ERR_INVALID, std::string(who) + ": " + what + " repeats a card or holds a byte that is not a card (0..51); nothing was written for it");
    return RS_OK;
}

}  // namespace rs
